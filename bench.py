#!/usr/bin/env python3
"""bench.py -- ringGroth16 prover throughput on MI355X (BASELINE.json metric, headline configuration).

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times K steps and prints the headline line (metric, value, ms_per_step, ...).
--full adds the legs beyond that figure, each untimed and after the K steps: measured peaks, the per-kernel
profile and rooflines, the standalone NTT and dyadic legs, the post-run oracle check, the C3F leg, the other BASELINE
configurations and the CPU baseline (N > 1: the transport phases and the sharded oracle check).  --dump-outputs DIR writes
the proof of the last timed step as DIR/proof.npy (float64; every residue < 2^53, so the values are exact).

One step = one groth16::prover call (zk_proof_systems/groth16/groth16.tcc:70-115: the witness map and
all encoding inner products) of the HEADLINE statement: m = 2^16 constraints on the ring N = 8192,
L = 4 primes (preset C3), encodings N_enc = 8192, K = 4; synthetic chain R1CS x_i * x_{i+1} = x_{i+2}
(n_aux = m), proving key and assignment resident in HBM when the clock starts.

The 2^16-constraint key is 384 GiB and cannot be resident on one 288 GiB GPU, so the key is a TILED
SYNTHETIC CRS: every key vector is stored as a window of 2^logw uniformly random elements (2 MiB each)
and term t reads element t mod 2^logw (include/ringsnark_amd.h, crs_window).  Every term still streams a
2 MiB element from HBM at an address 32 GiB away from its previous use (windows are >= 100x larger than
the 256 MiB Infinity Cache), and prover cost is data independent, so the timing is that of the full key.
The witness map is the real m = 2^16 one.

For N > 1 the SAME statement is proven by N ranks (strong scaling): limbs first, then the ranks sharing
a limb split its NTT slots for the witness map and its terms for the inner products
(ringsnark_amd/dist.py).  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP64_PEAK_T = 39.3     # vector FP64 FMA issue peak, T lane-ops/s: 256 CUs x 64 lanes/clk x 2.4 GHz (MI355X_MICROARCH.md)
# kernels bounded by FP64 issue (LDS-resident transforms); everything else is bounded by HBM
FP64_KERNELS = ("tree_columns_kernel", "tree_wide_kernel", "tree_tiles_generic_kernel", "h_tile_kernel", "h_columns_kernel", "interp_columns_kernel",
                "sub_ntt_kernel", "sub_ntt_ct_kernel", "sub_ntt_wide_kernel", "plain_center_kernel")


def rocprof_name(name):
    """Profile-record name -> prefix of the kernel name rocprofv3 prints (the library records `<name>` such that
    `rs::<name>` is that prefix, template arguments included where several instantiations exist)."""
    return "rs::" + name


def load_pmc(kind, preset, m):
    """The newest committed counter file of this kind ("traffic" / "fp64") for (preset, m) -- and whether it was collected on
    the device-library sources of THIS tree (tools/pmc_*.py record ringsnark_amd._lib.source_hash()).  A file without the
    hash, or with another one, is NOT joined: the line then carries null and the reason (round-3 verdict, "What's weak" 8)."""
    from ringsnark_amd._lib import source_hash
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s_%s_m%d.json" % (kind, preset, m))))
    if not cands:
        return None, "no profiles/r*_pmc_%s_%s_m%d.json" % (kind, preset, m)
    path = cands[-1]
    d = json.load(open(path))
    here = source_hash()
    if d.get("source_hash") != here:
        return None, "%s was collected on library sources %s (commit %s), this tree is %s: re-run tools/collect_profiles.sh" % (
            os.path.basename(path), d.get("source_hash"), d.get("commit"), here)
    d["_file"] = os.path.basename(path)
    return d, None


MEASURED = {}  # rs_measure_peaks of this run: the second denominators of SURVEY.md 8(d)


def measured_hbm():
    """The HBM denominator measured in this run: the BEST of the three streaming shapes (copy, read only, in place) -- the
    strictest one; 0 when nothing was measured."""
    return max(MEASURED.get("hbm_copy_gbs", 0.0), MEASURED.get("hbm_read_gbs", 0.0), MEASURED.get("hbm_inplace_gbs", 0.0))


def kernel_roofline(k, pmc, fp64_pmc=None, stale=None):
    """Roofline object of one per-kernel record from rs_profile_read (live HIP events on the launch stream).
    pmc: profiles/*_pmc_traffic_*.json (HBM bytes per kernel); fp64_pmc: profiles/*_pmc_fp64_*.json (SQ opcode counters per
    launch, tools/pmc_fp64.py) -- both from rocprofv3 passes of this very command, joined by the kernel name rocprofv3 prints."""
    sec = k["total_ms"] * 1e-3
    fp64 = any(k["name"].startswith(p) for p in FP64_KERNELS)
    out = {"kernel": k["name"], "launches": k["launches"], "avg_launch_ms": round(k["total_ms"] / max(1, k["launches"]), 4)}
    if fp64:
        ach = k["fp64_ops"] / sec / 1e12
        out.update({"bound": "fp64-issue", "achieved": round(ach, 2), "peak": FP64_PEAK_T, "unit": "T lane-op/s",
                    "frac": round(ach / FP64_PEAK_T, 4), "fp64_ops_per_launch": int(k["fp64_ops"] / max(1, k["launches"])),
                    "numerator": "model count of the library (8 FP64 instructions per lazy butterfly, 7 per pointwise modular multiply, "
                                 "v_rndne_f64 included; DESIGN.md section 3)",
                    "hbm_frac": round(k["alg_bytes"] / sec / 1e9 / HBM_PEAK_GBS, 4)})
        if MEASURED.get("fp64_fma_T"):  # against the v_fma_f64 rate this box sustains (clocks under FP64 load), not the spec sheet's
            out["frac_of_measured"] = round(ach / MEASURED["fp64_fma_T"], 4)
            out["peak_measured"] = round(MEASURED["fp64_fma_T"], 2)
        if fp64_pmc:
            fam = [v for n, v in fp64_pmc.get("kernels", {}).items() if n.startswith(rocprof_name(k["name"]))]
            if fam:  # per-proof totals of the counters over the live per-proof time of the same kernel (this step = one proof)
                cnt = sum(v["fp64_lane_ops"] for v in fam)
                valu = sum(v["valu_lane_ops"] for v in fam)
                out["counted"] = {
                    "source": "SQ_INSTS_VALU_{ADD,MUL,FMA}_F64 x 64 per proof (rocprofv3 --pmc, profiles/" + fp64_pmc.get("_file", "?") + ", collected on the "
                              "library sources of this tree: hash " + str(fp64_pmc.get("source_hash")) + ") over this run's time; "
                              "v_rndne_f64 has no opcode counter and is NOT in this figure (one per modular multiply: the model count minus ~1/8)",
                    "fp64_lane_ops_per_proof": int(cnt), "valu_lane_ops_per_proof": int(valu),
                    "launches_per_proof": round(sum(v["launches_per_proof"] for v in fam), 1),
                    "achieved": round(cnt / sec / 1e12, 2), "frac": round(cnt / sec / 1e12 / FP64_PEAK_T, 4),
                    "valu_issue_frac": round(valu / sec / 1e12 / FP64_PEAK_T, 4)}
    else:
        ach = k["alg_bytes"] / sec / 1e9
        out.update({"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4)})
        if measured_hbm():  # against the best streaming bandwidth measured in this run (copy / read only / in place)
            out["frac_of_measured"] = round(ach / measured_hbm(), 4)
            out["peak_measured"] = round(measured_hbm(), 1)
    if fp64 and "counted" not in out:
        out["counted"] = None
        out["counted_reason"] = (stale or {}).get("fp64") or "kernel not in the counter file"
    out["algorithmic_bytes_per_launch"] = int(k["alg_bytes"] / max(1, k["launches"]))
    # HBM traffic from the PMC passes (FETCH_SIZE x2 + WRITE_SIZE; tools/pmc_summary.py), same configuration,
    # keyed by the exact kernel family; null when the committed file does not hold this kernel
    traffic = None
    if pmc:
        fam = [v for n, v in pmc.get("kernels", {}).items() if n.startswith(rocprof_name(k["name"]))]
        if fam:
            traffic = int(sum(v["hbm_bytes"] for v in fam) / max(1, sum(v["launches_per_proof"] for v in fam)))
    out["traffic"] = traffic
    if traffic is not None:  # what the memory system actually moved per second (counter traffic over the live launch time)
        out["traffic_gbs"] = round(traffic * max(1, k["launches"]) / sec / 1e9, 1)
        if measured_hbm():
            out["traffic_frac_of_measured"] = round(out["traffic_gbs"] / measured_hbm(), 4)
    if traffic is None:
        out["traffic_reason"] = (stale or {}).get("traffic") or "kernel not in the counter file"
    return out


# post-run check (untimed): tests/proof_check.py -- witness-map identities on sampled columns and full proof
# slabs recomputed by the CPU oracle
from tests.proof_check import groth16_check as post_run_check  # noqa: E402


PRIME_CLASS = {
    "C3": "ring primes exactly as the reference's recipe yields them (default_double_batching_modulus(8192, 8192), seal/seal_util.hpp:20-32, "
          "examples/example_SEAL.cpp:15-22: q_i = 1 mod 2N = 2^14 only, 2-adicity 15, 15, 14, 14), i.e. what a SEAL-produced headline key has "
          "(SURVEY.md 8(d) C3); the witness map's transforms longer than 2^14 / 2^15 are INCOMPLETE (csrc/witness_inc.hpp)",
    "C3F": "'friendly' ring primes q_i = 1 mod 2^20 (a custom coeff_modulus, valid in the reference: the fields have roots of unity of order 2M "
           "and every transform of the witness map is complete) -- the preset rounds 1-5 quoted the headline on; an extra leg since round 6",
}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): this process starts the N ranks -- one process per
    GPU under torch.distributed.run, rendezvous on 127.0.0.1 -- as CHILDREN, before anything here has touched the GPU
    (importing torch does not initialise HIP; nothing above calls into it), passes their output through (rank 0 prints the
    one JSON line) and returns their exit code.  No exec, no retry: a failed rank means a non-zero exit."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def single_gpu_leg(preset, m, logw, steps, warmup, check):
    """The same headline statement on another preset (one GPU): time, phases, top kernels and the post-run oracle check."""
    from ringsnark_amd.device import Device
    prm = P.preset(preset)
    dev = Device(prm, 0)
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 1007)
    dev.chain_assignment(asg, m)
    W = 1 << logw
    pk = {k: dev.fill_uniform(dev.enc_empty(min(W, T)), 1, 1013 + i)
          for i, (k, T) in enumerate((("s_pows", m + 1), ("delta_ts", m + 1), ("delta_mid", cs.n_aux)))}
    pk["alpha"], pk["beta"] = dev.fill_uniform(dev.enc_empty(), 1, 1016), dev.fill_uniform(dev.enc_empty(), 1, 1017)
    window = W if W < m else 0
    proof = None
    for _ in range(warmup):
        proof = dev.groth16_prove(dcs, pk, asg, want_empty=False, window=window)[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = dev.groth16_prove(dcs, pk, asg, want_empty=False, window=window)[0]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dev.set_profiling(True)
    dev.profile_read()
    proof = dev.groth16_prove(dcs, pk, asg, want_empty=False, window=window)[0]
    torch.cuda.synchronize()
    timings, stats = dev.last_timings(), dev.profile_read()
    dev.set_profiling(False)
    out = {"preset": prm.name, "primes": PRIME_CLASS.get(prm.name, prm.notes), "steps": steps, "warmup": warmup,
           "ms_per_step": round(elapsed / steps * 1e3, 3), "value": round(m * steps / elapsed, 1), "unit": "constraints/s",
           "phase_ms": {"witness_map": round(timings["witness_ms"], 3), "msm": round(timings["msm_ms"], 3)},
           "kernels": [{"name": k["name"], "ms": round(k["total_ms"], 2), "launches": k["launches"]} for k in stats[:6]]}
    if check:
        ok, info = post_run_check(dev, prm, cs, dcs, asg, pk, proof, m, window or None, n_slabs=3)
        out["check"] = dict(info, ok=ok)
    del proof, asg, pk, dcs, dev
    torch.cuda.empty_cache()
    return out



def rinocchio_leg(preset, steps=3, logm=None, logw=None, logreg=False, check=True):
    """Rinocchio prover (rinocchio.tcc:75-190) on another BASELINE configuration's shape, one GPU: configs[3]'s ring shape
    (preset C4: N = 16384, 6 ring primes, N_enc = 16384, K = 8) on a chain circuit of 2^logm constraints with a tiled key
    -- the configuration's 2^18 constraints need a 9 TiB key -- or configs[4]: the circuit of the reference's
    benchmarks/bench_logistic_regression_inference.cpp (1031 constraints, whole key) on its own parameters (preset C5) or on
    the ring BASELINE.json names for it (preset C3: N = 8192, 4 primes).  ZK blinding on."""
    from ringsnark_amd.device import Device
    prm = P.preset(preset)
    dev = Device(prm, 0)
    if logreg:
        cs = R.logreg_r1cs(prm.q, 256)
        inputs = dev.fill_uniform(dev.ring_empty(4 * 256), 0, 41)
        asg = R.logreg_assignment(256, inputs, dev.ring_mul, dev.ring_add, dev.ring_mul_scalar)
        W = 0
    else:
        cs = R.chain_r1cs(1 << logm, prm.q)
        asg = dev.ring_empty(cs.m + 2)
        dev.fill_uniform(asg[:2], 0, 7)
        dev.chain_assignment(asg, cs.m)
        W = 1 << logw
    nk = (lambda T: min(T, W) if W else T)
    pk = {"s_pows": dev.fill_uniform(dev.enc_empty(nk(cs.m + 1)), 1, 22), "alpha_s_pows": dev.fill_uniform(dev.enc_empty(nk(cs.m + 1)), 1, 23),
          "beta_prods": dev.fill_uniform(dev.enc_empty(nk(cs.n_aux)), 1, 24)}
    for i, k in enumerate(("beta_rv_ts", "beta_rw_ts", "beta_ry_ts")):
        pk[k] = dev.fill_uniform(dev.enc_empty(), 1, 25 + i)
    ds = [dev.fill_uniform(dev.ring_empty(), 0, 30 + k) for k in range(3)]
    dcs = dev.r1cs(cs)
    for _ in range(2):
        dev.rinocchio_prove(dcs, pk, asg, *ds, window=W)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dev.rinocchio_prove(dcs, pk, asg, *ds, window=W)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    dev.set_profiling(True)
    dev.profile_read()
    proof = dev.rinocchio_prove(dcs, pk, asg, *ds, window=W)[0]
    torch.cuda.synchronize()
    tm, stats = dev.last_timings(), dev.profile_read()
    dev.set_profiling(False)
    chk = None
    if check:  # untimed: witness-map identities on sampled columns (ZK patch included) + a proof slab by the CPU oracle
        from tests.proof_check import rinocchio_check
        ok, info = rinocchio_check(dev, prm, cs, dcs, asg, pk, proof, cs.m, ds)
        chk = dict(info, ok=ok)
    out = {"preset": prm.name, "shape": "ring N=%d L=%d, encodings N_enc=%d K=%d" % (prm.N, prm.L, prm.N_enc, prm.K), "constraints": cs.m,
           "key_window": W or None, "ms_per_proof": round(dt * 1e3, 3), "value": round(cs.m / dt, 1), "unit": "constraints/s",
           "phase_ms": {"witness_map": round(tm["witness_ms"], 3), "msm": round(tm["msm_ms"], 3)},
           "kernels": [{"name": k["name"], "ms": round(k["total_ms"], 2)} for k in stats[:4]]}
    out["check"] = chk if chk is not None else "unchecked"
    del asg, pk, dcs, dev, proof
    torch.cuda.empty_cache()
    return out


def dyadic_leg(dev, prm, reps=100, gib=1.0):
    """SURVEY.md 8(d) rows a2 / a8 and the reference's own micro-timings (microbench.cpp:157-205: scalar x ring, ring + ring,
    ring x ring, encode + encrypt, decrypt + decode; 100 repetitions, mean microseconds).  Two figures per dyadic op:
    the HBM roofline of a LARGE batch (`gib` GiB per operand: algorithmic 16 or 24 bytes per residue against 8 TB/s and against
    the best streaming rate rs_measure_peaks found in this run) and the time of ONE element per call as the reference measures it
    (launch-latency bound on a GPU).  Encode / decode: microseconds per EncodingElem in a batch of 64 and alone."""
    from ringsnark_amd import _lib
    lib, h = dev.lib, dev.h
    ptr = lambda t: t.data_ptr()

    def timed(fn, n=reps):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()  # the library launches on torch's current stream (device.py passes it down)
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # microseconds per call

    def roof(us, nbytes):
        gbs = nbytes / us / 1e3
        o = {"us_per_launch": round(us, 2), "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4)}
        if measured_hbm():
            o["frac_of_measured"] = round(gbs / measured_hbm(), 4)
        return o

    out = {"bound": "hbm", "preset": prm.name, "reps": reps,
           "shape": "ring N=%d L=%d (%d-byte elements), encodings N_enc=%d K=%d" % (prm.N, prm.L, prm.ring_words * 8, prm.N_enc, prm.K),
           "reference": "microbench.cpp:157-205 (NUM_REPEATS = 100, mean microseconds per call on one element)"}
    T = max(1, int(gib * 2**30) // (prm.ring_words * 8))
    a = dev.fill_uniform(dev.ring_empty(T), 0, 51)
    b = dev.fill_uniform(dev.ring_empty(T), 0, 52)
    o = torch.empty_like(a)
    st = dev.stream()
    words = T * prm.ring_words
    ops = {"ring_mul_scalar (A x R)": (lambda n: _lib.check(lib.rs_ring_mul_scalar(h, ptr(o), ptr(a), 3, n, st)), 16),
           "ring_add (R + R)": (lambda n: _lib.check(lib.rs_ring_add(h, ptr(o), ptr(a), ptr(b), n, st)), 24),
           "ring_mul (R x R)": (lambda n: _lib.check(lib.rs_ring_mul(h, ptr(o), ptr(a), ptr(b), n, st)), 24)}
    for name, (fn, bpr) in ops.items():
        big = roof(timed(lambda: fn(T), 20), words * bpr)
        big["elements_per_launch"] = T
        big["algorithmic_bytes_per_residue"] = bpr
        big["us_per_element_in_batch"] = round(big["us_per_launch"] / T, 4)
        big["us_one_element_per_call"] = round(timed(lambda: fn(1)), 2)
        out[name] = big
    del a, b, o
    Te = max(1, int(gib * 2**30) // (prm.enc_words * 8))
    ea = dev.fill_uniform(dev.enc_empty(Te), 1, 53)
    eb = dev.fill_uniform(dev.enc_empty(Te), 1, 54)
    eo = torch.empty_like(ea)
    fn = lambda n: _lib.check(lib.rs_enc_add(h, ptr(eo), ptr(ea), ptr(eb), n, st))
    big = roof(timed(lambda: fn(Te), 20), Te * prm.enc_words * 24)
    big.update(elements_per_launch=Te, algorithmic_bytes_per_residue=24, us_per_element_in_batch=round(big["us_per_launch"] / Te, 4),
               us_one_element_per_call=round(timed(lambda: fn(1)), 2))
    out["enc_add (EncodingElem += EncodingElem, seal_ring.tcc:479-506)"] = big
    del ea, eb, eo
    # encode / decode: a ternary secret key in NTT form (any key times the same; a real one keeps the noise guard of decode quiet)
    rng = np.random.RandomState(7)
    s_coef = rng.randint(-1, 2, prm.N_enc)
    sk = torch.empty((prm.K, prm.N_enc), dtype=torch.int64, device=dev.device)
    for j, Qj in enumerate(prm.Q):
        sk[j] = torch.from_numpy(np.mod(s_coef, Qj).astype(np.int64)).to(dev.device)
        dev.ntt(sk[j:j + 1], _lib.RS_MOD_COEFF, j)
    rings = dev.fill_uniform(dev.ring_empty(64), 0, 55)
    enc = dev.enc_encode(sk, rings, 9)
    dec = dev.enc_decode(sk, enc)
    ok = bool((dec == rings).all())
    e_b = timed(lambda: dev.enc_encode(sk, rings, 9), 20)
    d_b = timed(lambda: dev.enc_decode(sk, enc), 20)
    e_1 = timed(lambda: dev.enc_encode(sk, rings[0], 9), 50)
    d_1 = timed(lambda: dev.enc_decode(sk, enc[0]), 50)
    out["encode / decode (EncodingElem::encode, ::decode: L ciphertexts per element; seal_ring.tcc:324-359, 435-477)"] = {
        "encode_us_per_element_in_batch_of_64": round(e_b / 64, 2), "decode_us_per_element_in_batch_of_64": round(d_b / 64, 2),
        "encode_us_one_element_per_call": round(e_1, 2), "decode_us_one_element_per_call": round(d_1, 2),
        "round_trip_equal": ok, "note": "each call ends with a stream synchronisation (the entry points return host-visible status)"}
    del rings, enc, dec, sk
    torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------------------------------------------
# CPU baseline: the oracle (a port of the reference's algorithm) on a bounded sample
# ---------------------------------------------------------------------------------------------------
def cpu_baseline(prm, m, n_aux):
    """The CPU restatement of the reference's algorithm timed on this box's host cores with the arithmetic Microsoft SEAL
    publishes for it (oracle/librs_oracle_fast.so: Harvey lazy NTT with Shoup quotients, Barrett products -- NOT the
    `%`-based checker, which would understate a SEAL build; tests/test_oracle.py holds the two bit-identical):
    1 thread (what groth16::prover uses -- no OpenMP in groth16.tcc:70-115) and all cores (OpenMP over terms / slots,
    SURVEY.md 8(d)).  MSM: inner-product terms at full ring shape, >= 64 terms per thread.  Witness map: the reference's
    O(m^2) algorithm measured at a small m_s on a few slots and scaled by (m/m_s)^2 x (N L / slots): its cost is exactly
    quadratic in m and linear in slots."""
    from oracle import fastcpu as F
    from oracle import oracle as O
    from tests import helpers as H

    ctx = H.oracle_ctx(prm)  # input generators only
    fast = F.FastCtx(prm.N, prm.q, prm.N_enc, prm.Q)
    nthr = F.max_threads()
    terms_total = 4 * m + (m + 1) + n_aux  # groth16.tcc:89-112
    win = 16
    encs = ctx.random_enc(1, win)
    T1, TN = 256, max(1024, 64 * nthr)

    def msm_rate(threads, T):
        rings = ctx.random_ring(2, T)
        t0 = time.perf_counter()
        fast.inner_product(encs, rings, threads=threads, window=win)
        return (time.perf_counter() - t0) / T  # seconds per term

    def witness_time(threads, m_s, slots):
        cs = R.chain_r1cs(m_s, prm.q[:1])
        q = prm.q[0]
        rng = np.random.RandomState(3)
        asg = np.zeros((m_s + 2, slots), dtype=np.uint64)
        asg[0] = rng.randint(1, 2**31, slots)
        asg[1] = rng.randint(1, 2**31, slots)
        for i in range(m_s):
            asg[i + 2] = (asg[i].astype(object) * asg[i + 1].astype(object) % q).astype(np.uint64)
        best = None
        for fn in (F.witness_map, O.witness_map):  # Barrett build and `%` build (128-by-64-bit hardware divide): whichever this host runs faster
            t0 = time.perf_counter()
            fn(q, H.oracle_cs(cs), 0, asg, threads=threads)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * (m / m_s) ** 2 * (prm.N * prm.L / slots)

    t1_term = msm_rate(1, T1)
    tN_term = msm_rate(0, TN)
    slots_n = max(256, 32 * nthr)
    w1 = witness_time(1, 128, 256)
    wN = witness_time(0, 128, slots_n)
    one = m / (w1 + terms_total * t1_term)
    allc = m / (wN + terms_total * tN_term)
    return {
        "value": allc, "unit": "constraints/s", "cores": nthr, "kind": "port", "nproc": os.cpu_count(),
        "arithmetic": "SEAL-style: Harvey lazy NTT with Shoup quotients, Barrett 128-bit products (oracle/rs_fastcpu.c, "
                      "rs_oracle.c -DRSO_FAST_MULMOD); gcc -O3 -march=native -fopenmp",
        "sample": "inner_product on %d terms (1 thread) / %d terms (%d threads, %d per thread) at full ring shape, scaled to the %d "
                  "terms of one proof; the reference's O(m^2) witness map at m=128 on 256 / %d slots (the faster of the Barrett and the "
                  "hardware-divide builds), scaled x(m/128)^2 x(N L/slots)"
                  % (T1, TN, nthr, TN // max(1, nthr), terms_total, slots_n),
        "one_thread": {"value": one, "cores": 1, "msm_s_per_proof": terms_total * t1_term, "witness_s_per_proof": w1},
        "all_cores": {"value": allc, "cores": nthr, "msm_s_per_proof": terms_total * tN_term, "witness_s_per_proof": wN},
        "msm_only": {"one_thread": m / (terms_total * t1_term), "all_cores": m / (terms_total * tN_term), "unit": "constraints/s"},
        "witness_only": {"one_thread": m / w1, "all_cores": m / wN, "unit": "constraints/s", "note": "extrapolated from m=128"},
    }


def dump_outputs(out_dir, proof):
    """--dump-outputs: the proof the last timed step returned ([3, L, 2, K, N_enc] residues, 6 MiB at the headline) as
    out_dir/proof.npy in float64.  Every residue is below its modulus < 2^53, so the conversion is exact."""
    words = proof.detach().cpu().numpy()
    assert words.min() >= 0 and words.max() < 2**53, "proof residues out of range"
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "proof.npy"), words.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", default="C3")
    ap.add_argument("--logm", type=int, default=16, help="log2 of the constraints of the statement (all GPUs together)")
    ap.add_argument("--logw", type=int, default=None,
                    help="log2 of the key window (stored elements per key vector) per GPU; default: every rank stores its WHOLE "
                         "term range of the key when that fits beside the prover's workspaces (N >= 4 at the headline), else 2^14")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-ntt", action="store_true", help="skip the standalone NTT bandwidth leg (profiling passes)")
    ap.add_argument("--no-friendly-primes", "--no-recipe-primes", dest="no_friendly_primes", action="store_true",
                    help="skip the second leg on preset C3F (ring primes = 1 mod 2^20: complete transforms)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short Rinocchio legs at the shapes of BASELINE configs[3] / configs[4]")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure (peaks, per-kernel rooflines, NTT / dyadic legs, oracle check, "
                         "C3F, other configurations, CPU baseline; N > 1: transport phases and check); the --no-* options apply to these")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the proof of the last timed step as DIR/proof.npy (float64, exact)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))  # plain `python bench.py --gpus N`: start the N ranks, relay their line and exit code
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N ranks with torch.distributed.run --nproc-per-node N, "
                 "or run plain `python bench.py --gpus N`, which launches them itself)" % (args.gpus, world))
    import torch.distributed as dist

    from ringsnark_amd import dist as RD
    from ringsnark_amd.device import Device

    # Developer rehearsal of the N > 1 path on a single-GPU box: RINGSNARK_BENCH_REHEARSAL=1 puts every
    # rank on cuda:0 and uses gloo (the numbers mean nothing; the code path is the production one).
    rehearsal = os.environ.get("RINGSNARK_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            import datetime
            # a collective that never completes (a transport this code has not met on hardware) must end the run with an
            # error after five minutes -- the NCCL watchdog aborts the ranks -- not hold the node
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=datetime.timedelta(seconds=300))

    prm = P.preset(args.preset)
    m = 1 << args.logm
    plan = RD.make_plan(world, rank, prm.L)
    prm_local = P.RingParams(prm.N, [prm.q[i] for i in plan.limbs], prm.N_enc, prm.Q, name=prm.name)
    setup = {}
    t_s = time.perf_counter()
    dev = Device(prm_local, local_rank)
    setup["context_ms"] = round((time.perf_counter() - t_s) * 1e3, 1)  # rs_ctx_create: transform tables of every prime, index map
    if world == 1 and args.full:
        try:
            MEASURED.update(dev.measure_peaks())
        except Exception as e:  # e.g. the two 2 GiB buffers do not fit: the line then carries no measured denominators
            setup["measured_peaks_error"] = str(e)
            torch.cuda.empty_cache()
    cs = R.chain_r1cs(m, prm_local.q)
    t_s = time.perf_counter()
    dcs = dev.r1cs(cs)
    setup["r1cs_upload_ms"] = round((time.perf_counter() - t_s) * 1e3, 1)
    n_aux = cs.n_aux
    # synthetic inputs, generated on device (seeded per (limb group, role))
    seed0 = 1000 * (plan.limb_group + 1)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, seed0 + 7)
    dev.chain_assignment(asg, m)
    # Key: every rank stores, per key vector, a window of at most 2^logw elements of its limbs; a rank whose
    # term range is shorter than the window stores exactly its range (TiledKey maps a logical term to storage).
    ranges = RD.groth16_key_ranges(plan, m, n_aux)
    if args.logw is not None:
        W = 1 << args.logw
    else:
        # bytes of this rank's real key share: its limbs of the terms it reads; the prover's own buffers (assignment,
        # five coefficient vectors, column chunk, multi-pass workspaces, MSM scratch) take up to ~125 GiB per rank
        share = sum(hi - lo for lo, hi in ([(0, m + 1), (0, m + 1), (0, n_aux)] if world == 1 else ranges.values()))
        whole_fits = share * prm_local.enc_words * 8 <= 140 * 2**30
        W = (1 << 40) if whole_fits else (1 << 14)

    def key_vector(name, T, seed):
        lo, hi = (0, T) if world == 1 else ranges[name]
        stored = min(max(hi - lo, 1), W)
        store = dev.fill_uniform(dev.enc_empty(stored), 1, seed + 100 * plan.term_shard)
        return RD.TiledKey(store, lo, hi, T)

    pk = {
        "s_pows": key_vector("s_pows", m + 1, seed0 + 13),
        "delta_ts": key_vector("delta_ts", m + 1, seed0 + 14),
        "delta_mid": key_vector("delta_mid", n_aux, seed0 + 15),
        "alpha": dev.fill_uniform(dev.enc_empty(), 1, seed0 + 16),
        "beta": dev.fill_uniform(dev.enc_empty(), 1, seed0 + 17),
    }
    stored_gib = sum(v.store.numel() * 8 for v in pk.values() if isinstance(v, RD.TiledKey)) / 2**30
    tiled = any(isinstance(v, RD.TiledKey) and v.window for v in pk.values())
    term_group = RD.groups_for(plan) if world > 1 else None
    backend = RD.DeviceBackend(dev)
    pk1 = {k: (v.store if isinstance(v, RD.TiledKey) else v) for k, v in pk.items()}
    window1 = W if (world == 1 and tiled) else 0
    proof = [None]

    def step():
        if world == 1:
            proof[0] = dev.groth16_prove(dcs, pk1, asg, want_empty=False, window=window1)[0]
        else:
            proof[0] = RD.groth16_prove_sharded(backend, plan, term_group, dcs, pk, asg, m, cs.n_inputs, n_aux)
        return proof[0]

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the FIRST proof pays for what a prover process does once per (context, m): the witness-map plan (product-tree spectra,
    # rev(Z)^-1 by Newton iteration on the host), the io-vector cache of the circuit, first-call workspace allocations.
    # Excluded from the timed region, reported here (excluded work is "reported separately").
    fence()
    t_s = time.perf_counter()
    step()
    fence()
    first_ms = (time.perf_counter() - t_s) * 1e3
    for _ in range(max(0, args.warmup - 1)):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev.device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    ms_per_step = elapsed / args.steps * 1e3
    value = m * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, proof[0])
    setup["first_proof_ms"] = round(first_ms, 1)
    setup["first_proof_extra_ms"] = round(first_ms - ms_per_step, 1)
    setup["note"] = ("not in the timed region: context creation, R1CS upload, and what the first proof of a (context, m) pays once -- witness-map "
                     "plan and tables built on the host, the circuit's io-vector cache, workspace allocations" + (" (a warm-up step here)" if args.warmup else ""))

    # ---- N > 1: one more (untimed) step with the collectives bracketed by HIP events on the streams they run on: what each
    # transport phase moved and how long it took on this rank, and the device time of the rank's own kernels
    transport_phases = None
    if world > 1 and args.full:
        RD.STATS.reset(True)
        dev.set_profiling(True)
        dev.profile_read()
        fence()
        t_s = time.perf_counter()
        step()
        fence()
        step_ms = (time.perf_counter() - t_s) * 1e3
        transport_phases = RD.STATS.read()
        RD.STATS.reset(False)
        kstats = dev.profile_read()
        dev.set_profiling(False)
        transport_phases["rank0_step_ms"] = round(step_ms, 3)
        transport_phases["rank0_kernel_ms"] = round(sum(k["total_ms"] for k in kstats), 3)
        transport_phases["rank0_top_kernels"] = [{"name": k["name"], "ms": round(k["total_ms"], 2)} for k in kstats[:5]]
        transport_phases["note"] = ("rank 0, one untimed step after the timed ones: bytes this rank sent + received per collective and the time between "
                                    "HIP events around it on the stream it ran on (the slot -> term exchange runs on a side stream under the next "
                                    "sub-range's witness map, so its ms overlap the kernels'); GB_per_s = bytes / ms")

    # ---- N > 1: a small statement over the SAME process group and plan shape against the one-process CPU oracle, bit for bit
    # (tests/dist_check.py): no multi-GPU run has been measured by any round, so a bench line from one must say that the
    # transport it timed also carries a correct proof (the headline-size proof itself is checked at N = 1)
    transport_check = None
    if world > 1 and args.full and not args.no_check:
        from tests.dist_check import sharded_proof_matches_oracle
        t_s = time.perf_counter()
        tc_preset, tc_m = ("toyC3" if prm.L == 4 else "toy"), 12
        ok_t = sharded_proof_matches_oracle(rank, world, local_rank, tc_preset, tc_m, None, "groth16", False)
        fence()
        transport_check = {"ok": ok_t, "what": "groth16_prove_sharded on preset %s (the headline's ring primes on a 32-slot ring), %d constraints, the same "
                                               "ranks / plan shape / witness split / relays as the timed proof, equal to the one-process oracle proof bit for bit"
                                               % (tc_preset, tc_m), "seconds": round(time.perf_counter() - t_s, 1)}

    # ---- per-kernel device time of one more (untimed) step: HIP events on the launch stream inside the library
    roofline = mac_roofline = timings = kernels = None
    if world == 1 and args.full:
        stale = {}
        pmc, stale["traffic"] = load_pmc("traffic", prm.name, m)
        fp64_pmc, stale["fp64"] = load_pmc("fp64", prm.name, m)
        dev.set_profiling(True)
        dev.profile_read()
        step()
        torch.cuda.synchronize()
        timings = dev.last_timings()
        stats = dev.profile_read()
        dev.set_profiling(False)
        tot = sum(k["total_ms"] for k in stats) or 1.0
        kernels = [{"name": k["name"], "ms": round(k["total_ms"], 2), "share": round(k["total_ms"] / tot, 4),
                    "launches": k["launches"]} for k in stats[:10]]
        if stats:
            roofline = kernel_roofline(stats[0], pmc, fp64_pmc, stale)  # the dominant kernel by time
        mac = [k for k in stats if k["name"].startswith("mac_kernel")]
        if mac:
            mac_roofline = kernel_roofline(mac[0], pmc, fp64_pmc, stale)

    # ---- the standalone transform (row a4), HBM bound by design: 16 bytes per coefficient per transform, on 4 GiB
    ntt_roofline = None
    if world == 1 and args.full and not args.no_ntt:
        from ringsnark_amd import _lib
        reps, blocks = 10, 5

        def ntt_leg(d, p, gib=4):
            """forward / inverse GB/s of the standalone transform of context d on a 4 GiB batch (algorithmic 16 B / coefficient)"""
            batch = (gib << 30) // (p.N_enc * 8)
            polys = torch.empty((batch, p.N_enc), dtype=torch.int64, device=d.device).random_(0, int(p.Q[0]))
            res = []
            for inverse in (False, True):
                for _ in range(10):  # steady state: the first launches after an idle stretch run at a lower clock
                    d.ntt(polys, _lib.RS_MOD_COEFF, 0, inverse=inverse)
                rates = []
                for _ in range(blocks):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()  # the library launches on torch's current stream (device.py passes it down)
                    for _ in range(reps):
                        d.ntt(polys, _lib.RS_MOD_COEFF, 0, inverse=inverse)
                    e1.record()
                    torch.cuda.synchronize()
                    rates.append(batch * p.N_enc * 16 * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
                res.append(sorted(rates)[len(rates) // 2])  # median of the blocks
            del polys
            o = {"bound": "hbm", "kernel": "forward NTT, %d transforms of %d points per launch (%d GiB in place, preset %s), median of %d blocks of %d launches"
                                           % (batch, p.N_enc, gib, p.name, blocks, reps),
                 "achieved": round(res[0], 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(res[0] / HBM_PEAK_GBS, 4),
                 "inverse": {"achieved": round(res[1], 1), "frac": round(res[1] / HBM_PEAK_GBS, 4)}}
            if measured_hbm():
                o["frac_of_measured"] = round(res[0] / measured_hbm(), 4)
                o["inverse"]["frac_of_measured"] = round(res[1] / measured_hbm(), 4)
            return o

        ntt_roofline = ntt_leg(dev, prm)
        # the same at 16384 points (the reference's micro-benchmark length, microbench.cpp:13-14; the encoding degree of
        # BASELINE configs[3] / [4]) on preset C4's 48-bit data primes: a second, small context
        p16 = P.preset("C4")
        d16 = Device(p16, local_rank)
        ntt_roofline["at_16384_points"] = ntt_leg(d16, p16)
        del d16
        # ... and on the INTEGER arithmetic: the reference's own micro-benchmark parameters (microbench.cpp:13-14,33-36: N = 16384,
        # coefficient primes of {59, 60, 60} bits), Montgomery products -- ALU-bound: a butterfly is one Montgomery product, so
        # beside the HBM fraction the line carries products/s against the rate rs_measure_peaks found for that very product
        p60 = P.preset("micro60")
        d60 = Device(p60, local_rank)
        leg = ntt_leg(d60, p60, gib=1)
        logn = p60.N_enc.bit_length() - 1
        for o, gbs in ((leg, leg["achieved"]), (leg["inverse"], leg["inverse"]["achieved"])):
            prods = gbs * 1e9 / 16.0 * logn / 2.0  # coefficients/s x log2(n)/2 butterflies per coefficient
            o["montgomery_products_G_per_s"] = round(prods / 1e9, 1)
            if MEASURED.get("int_montmul_G"):
                o["frac_of_measured_product_rate"] = round(prods / 1e9 / MEASURED["int_montmul_G"], 4)
        leg["bound"] = "integer ALU (v_mad_u64_u32: no 64x64 multiplier on gfx950)"
        ntt_roofline["micro60_integer_arithmetic"] = leg
        del d60

    # ---- rows a2 / a8 of SURVEY 8(d) and the reference's micro-timings: dyadic ring ops, enc_add, encode / decode
    dyadic = None
    if world == 1 and args.full and not args.no_ntt:
        try:
            dyadic = dyadic_leg(dev, prm)
            p60 = P.preset("micro60")  # microbench.cpp:13-14,33-36: N = 16384, {59, 60, 60}-bit primes -- the integer (Montgomery) arithmetic
            d60 = Device(p60, local_rank)
            dyadic["micro60_integer_arithmetic"] = dyadic_leg(d60, p60, gib=0.5)
            del d60
        except Exception as e:  # an extra leg must not cost the line
            dyadic = {"error": repr(e)}
        torch.cuda.empty_cache()

    # ---- untimed post-run check of the timed proof against the CPU oracle
    check = None
    if world == 1 and args.full and not args.no_check:
        pk.clear()  # the check releases the key (pk1 holds the last references) before it re-runs the witness map
        ok, info = post_run_check(dev, prm, cs, dcs, asg, pk1, proof[0], m, window1 or pk1["s_pows"].shape[0], n_slabs=3)
        check = dict(info, ok=ok)

    # ---- the same statement on "friendly" ring primes (preset C3F: = 1 mod 2^20, complete transforms; the headline of rounds 1-5), one GPU
    friendly = None
    if world == 1 and args.full and prm.name == "C3" and not args.no_friendly_primes:
        del proof[0]
        proof.append(None)
        pk.clear()
        pk1.clear()
        del asg, dcs, dev, backend
        torch.cuda.empty_cache()
        friendly = single_gpu_leg("C3F", m, min(14, W.bit_length() - 1), max(1, min(args.steps, 5)), 1, not args.no_check)

    # ---- the other BASELINE configurations' shapes, a few seconds each (extra keys, not the metric)
    other = None
    if world == 1 and prm.name == "C3" and friendly is not None and not args.no_other_configs:
        other = {"configs[1] (ringGroth16, 2^10 constraints, N=4096 L=2, N_enc=8192 K=4; whole 3 GiB key)": single_gpu_leg("C2", 1 << 10, 11, 20, 3, not args.no_check),
                 "configs[3] shape (Rinocchio, N=16384, 6 ring primes, K=8; 2^12 constraints, key window 2^9)": rinocchio_leg("C4", logm=12, logw=9, check=not args.no_check),
                 "configs[4] (Rinocchio, the reference's logistic-regression circuit and parameters: N=2048, one 54-bit prime, N_enc=16384 K=8)": rinocchio_leg("C5", steps=10, logreg=True, check=not args.no_check),
                 "configs[4] as BASELINE.json words it (the same circuit on N=8192, 4 primes: the headline's parameters)": rinocchio_leg("C3", steps=10, logreg=True, check=not args.no_check)}

    if rank == 0:
        key_gib = (3 * m + 2) * prm.enc_words * 8 / 2**30
        out = {
            "metric": "prover constraints/sec (ringGroth16, N=8192, 4 RNS primes)",
            "value": round(value, 1), "unit": "constraints/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "ringGroth16 prover (groth16.tcc:70-115), synthetic chain R1CS m=%d constraints (n_aux=m), ring N=%d L=%d, "
                                   "encodings N_enc=%d K=%d; %s; real m=%d witness map"
                                   % (m, prm.N, prm.L, prm.N_enc, prm.K,
                                      ("tiled synthetic CRS: %.0f GiB key stood in for by a resident window of 2^%d elements per key vector "
                                       "(%.0f GiB in HBM per GPU), term index wrapped" % (key_gib, W.bit_length() - 1, stored_gib)) if tiled else
                                      ("synthetic CRS %.0f GiB, %.0f GiB resident per GPU" % (key_gib, stored_gib)), m),
                       "preset": prm.name, "primes": PRIME_CLASS.get(prm.name, prm.notes), "constraints": m,
                       "key_window": (min(W, m + 1) if tiled else None),
                       "parallelism": "limbs%d x shards%d" % (plan.limb_groups, plan.term_shards)},
        }
        if world > 1:
            out["config"]["parallelism_detail"] = (
                "%d limb group(s) x %d rank(s) per group; witness map split: %s%s; inner products by terms inside a group, one "
                "all-reduce(SUM) of the partial encoding sums per group, one all-gather assembles the proof" % (
                    plan.limb_groups, plan.term_shards,
                    "none (each rank owns whole limbs and runs the fused prover)" if plan.term_shards == 1 else RD.WITNESS_SPLIT,
                    "" if plan.term_shards == 1 or RD.WITNESS_SPLIT != "slots" else
                    (", slot->term exchange relayed through the other groups" if RD.RELAY else ", slot->term exchange on the group's direct links")))
            out["transport"] = {"backend": dist.get_backend(), "ranks": dist.get_world_size(),
                                "rccl_ranks": dist.get_world_size() if dist.get_backend() == "nccl" else 0,
                                "devices_visible": torch.cuda.device_count(), "rehearsal_all_ranks_on_one_gpu": rehearsal,
                                "phases": transport_phases, "check": transport_check}
        out["setup"] = setup
        if MEASURED:
            out["measured_peaks"] = {"hbm_copy_gbs": round(MEASURED["hbm_copy_gbs"], 1), "hbm_read_gbs": round(MEASURED["hbm_read_gbs"], 1),
                                     "hbm_inplace_gbs": round(MEASURED["hbm_inplace_gbs"], 1), "fp64_fma_T": round(MEASURED["fp64_fma_T"], 2),
                                     "fp64_mulmod_G": round(MEASURED["fp64_mulmod_G"], 1), "int_montmul_G": round(MEASURED["int_montmul_G"], 1),
                                     "how": "rs_measure_peaks at the start of this run: 2 GiB streamed with 16-byte accesses three ways -- device-to-device copy, read only, in-place update (read + written bytes; each the best of four grid sizes, temporal and non-temporal accesses, the copy also hipMemcpyAsync); the HBM rooflines' `frac_of_measured` divides by the BEST of the three; v_fma_f64 "
                                            "lane-operations/s, exact-FP64 modular multiplies/s (6 instructions each), Montgomery products/s on a 60-bit prime; "
                                            "`frac_of_measured` in the rooflines divides by these, `frac` by the spec sheet"}
        if timings:
            out["phase_ms"] = {"witness_map": round(timings["witness_ms"], 3), "msm": round(timings["msm_ms"], 3)}
        if kernels:
            out["kernels"] = kernels
        if roofline:
            out["roofline"] = roofline
        if mac_roofline:
            out["mac_roofline"] = mac_roofline
        if ntt_roofline:
            out["ntt_roofline"] = ntt_roofline
        if dyadic:
            out["dyadic_roofline"] = dyadic
        if check is not None:
            out["check"] = check
        if friendly is not None:
            out["friendly_primes"] = friendly
        if other is not None:
            out["other_configs"] = other
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(prm, m, n_aux)
        print(json.dumps(out), flush=True)
    bad = (check is not None and not check["ok"]) or (friendly is not None and "check" in friendly and not friendly["check"]["ok"])
    for leg in (other or {}).values():
        bad = bad or (isinstance(leg.get("check"), dict) and not leg["check"]["ok"])
    if world > 1 and transport_check is not None:  # rank 0's verdict decides for every rank
        flag = torch.tensor([0 if (rank != 0 or transport_check["ok"]) else 1], dtype=torch.int64, device=dev.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        bad = bad or bool(flag.item())
    if world > 1:
        RD.release_buffers()  # the pooled receive / relay buffers of the re-shard live until released (dist.py)
        dist.destroy_process_group()
    if bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
