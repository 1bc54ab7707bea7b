"""rs_r1cs_check against the composition the ABI offered before it (DESIGN.md "R1CS satisfaction check").

Per shape -- chain_r1cs and wide_r1cs on C2 at m = 2^10 and on C3's ring at m = 2^13 -- on satisfied, fixed assignments:
  fused     one rs_r1cs_check call (host clock around the call; it synchronises), and the device time of its kernel from the
            library's own per-launch events (rs_set_profiling), in a pass of its own
  composed  3 x rs_r1cs_evaluate, rs_ring_mul, rs_ring_sub, rs_ring_is_zero (host clock; the last one synchronises), the
            four [m][L][N] scratch vectors allocated outside the timed region
Warm-up, then the two alternate; medians.  The fused kernel's rate is taken over the unique assignment bytes
n_vars * L * N * 8 and set against rs_measure_peaks().hbm_read_gbs of the same run.

usage: python tools/r1cs_check_probe.py [--out FILE] [--repeats 15] [--shapes C2:10,C3:13]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ringsnark_amd import _lib  # noqa: E402
from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402
from ringsnark_amd.device import Device, _ptr  # noqa: E402


def wide_assignment(dev, cs):
    """forward solve of wide_r1cs on the device: x_{i+2} = <a_i, (1, x)> * x_{i+1}"""
    x = dev.ring_empty(cs.n_vars)
    dev.fill_uniform(x[:2], 0, 5)
    rp, col, cf = cs.mats["a"]
    q0 = int(dev.prm.q[0])
    zero = torch.zeros_like(x[0])
    for i in range(cs.m):
        acc = zero
        for e in range(int(rp[i]), int(rp[i + 1])):
            c = int(cf[0, e])
            neg = c > q0 // 2  # a signed literal c < 0 is stored as q - |c|
            mag = q0 - c if neg else c
            if col[e] == 0:
                assert not neg
                acc = dev.ring_add_scalar(acc, mag)
            else:
                t = dev.ring_mul_scalar(x[int(col[e]) - 1], mag)
                acc = dev.ring_sub(acc, t) if neg else dev.ring_add(acc, t)
        x[i + 2] = dev.ring_mul(acc, x[i + 1])
    dev.sync()
    return x


def chain_assignment(dev, cs):
    x = dev.ring_empty(cs.n_vars)
    dev.fill_uniform(x[:2], 0, 5)
    dev.chain_assignment(x, cs.m)
    dev.sync()
    return x


def probe(dev, name, cs, asg, repeats, peaks):
    dcs = dev.r1cs(cs)
    m = cs.m
    lib, h, st = dev.lib, dev.h, dev.stream()
    rep = _lib.R1csReport()
    scratch = [dev.ring_empty(m) for _ in range(4)]
    zflags = (C.c_uint8 * m)()

    def fused():
        _lib.check(lib.rs_r1cs_check(h, dcs.h, _ptr(asg), None, C.byref(rep), st))
        return rep.n_violated == 0

    def composed():
        for k in range(3):
            _lib.check(lib.rs_r1cs_evaluate(h, dcs.h, k, _lib.RS_EVAL_FULL, _ptr(asg), _ptr(scratch[k]), st))
        _lib.check(lib.rs_ring_mul(h, _ptr(scratch[3]), _ptr(scratch[0]), _ptr(scratch[1]), m, st))
        _lib.check(lib.rs_ring_sub(h, _ptr(scratch[0]), _ptr(scratch[3]), _ptr(scratch[2]), m, st))
        _lib.check(lib.rs_ring_is_zero(h, _ptr(scratch[0]), m, zflags, st))
        return all(zflags)

    def timed(f):
        dev.sync()
        t = time.perf_counter()
        ok = f()
        return (time.perf_counter() - t) * 1e3, ok

    for _ in range(3):
        assert fused() and composed(), "the probe's assignment does not satisfy its system"
    tf, tc = [], []
    for _ in range(repeats):  # alternating: both see the same neighbours
        tf.append(timed(fused)[0])
        tc.append(timed(composed)[0])
    # the kernel alone: device events around the launch, in a pass of its own
    dev.set_profiling(True)
    dev.profile_read()
    for _ in range(repeats):
        fused()
    stats = [s for s in dev.profile_read() if s["name"] == "r1cs_check"]
    dev.set_profiling(False)
    kernel_ms = stats[0]["total_ms"] / stats[0]["launches"] if stats else float("nan")
    asg_bytes = cs.n_vars * dev.L * dev.N * 8
    rate = asg_bytes / (kernel_ms * 1e-3) / 1e9
    out = {"shape": name, "m": m, "n_vars": cs.n_vars, "N": dev.N, "L": dev.L, "nnz": [cs.nnz(n) for n in "abc"],
           "fused_call_ms": statistics.median(tf), "fused_call_ms_min_max": [min(tf), max(tf)],
           "composed_ms": statistics.median(tc), "composed_ms_min_max": [min(tc), max(tc)],
           "fused_kernel_ms": kernel_ms, "assignment_bytes": asg_bytes, "fused_kernel_gbs_over_assignment": rate,
           "fraction_of_hbm_read": rate / peaks["hbm_read_gbs"], "repeats": repeats}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--shapes", default="C2:10,C3:13")
    args = ap.parse_args()
    results = []
    for spec in args.shapes.split(","):
        preset, logm = spec.split(":")
        prm = P.preset(preset)
        dev = Device(prm)
        peaks = dev.measure_peaks()
        print(json.dumps({"preset": preset, "peaks": peaks}), flush=True)
        m = 1 << int(logm)
        for kind in ("chain", "wide"):
            cs = R.chain_r1cs(m, prm.q) if kind == "chain" else R.wide_r1cs(m, prm.q)
            asg = chain_assignment(dev, cs) if kind == "chain" else wide_assignment(dev, cs)
            results.append(probe(dev, "%s %s m=2^%s" % (preset, kind, logm), cs, asg, args.repeats, peaks))
            results[-1]["hbm_read_gbs"] = peaks["hbm_read_gbs"]
            del asg
        del dev
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
