"""rs_ring_inv_or_zero (ringsnark_amd/inverse.h) beside rs_ring_inv, whole calls on one MI355X.

Per preset -- C3 (N = 8192, L = 4, FP64) and C5 (N = 2048, L = 1, Montgomery) -- and per count (64 and 1024 elements):
  rs_ring_inv on clean input (the yardstick: one Fermat power per word), and rs_ring_inv_or_zero on clean input, with half of
  the slots zero, with a numerator, and strided with stride 3 in place in an is-zero assignment (Device.is_zero_fill).
Host clock around a call that synchronises (both calls download their flag or report); the calls alternate inside one
process, one warm-up round, then the median of 5 (min and max beside it).  GB/s over 16 bytes a word (24 with a numerator).

usage: python tools/inv_or_zero_time.py [--out profiles/inv_or_zero.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ringsnark_amd import _lib  # noqa: E402
from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd.device import Device  # noqa: E402

REPEATS, WARM = 5, 1
PRESETS = ("C3", "C5")
COUNTS = (64, 1024)


def units(dev, count, seed):
    """[count][L][N] on the device: uniform non-zero residues"""
    g = torch.Generator(device=dev.device)
    g.manual_seed(seed)
    return torch.stack([torch.randint(1, int(q), (count, dev.N), dtype=torch.int64, device=dev.device, generator=g) for q in dev.prm.q], dim=1).contiguous()


def measure(dev, count):
    """{case: (times in ms, bytes a word)} -- the five calls in turn, WARM + REPEATS rounds"""
    x = units(dev, count, 1)
    half = x.clone()
    half[:, :, 0::2] = 0
    num = units(dev, count, 2)
    out = torch.empty_like(x)
    asg = dev.ring_empty(1 + 3 * count)
    asg[0] = 1
    asg[1::3] = x
    dev.sync()

    def ring_inv():
        _lib.check(dev.lib.rs_ring_inv(dev.h, out.data_ptr(), x.data_ptr(), count, dev.stream()))

    def clean():
        _, rep = dev.ring_inv_or_zero(x, out=out)
        assert rep.n_zero == 0 and rep.clean, rep

    def half_zero():
        _, rep = dev.ring_inv_or_zero(half, out=out)
        assert rep.n_zero == count * dev.L * dev.N // 2 and rep.clean, rep

    def with_num():
        _, rep = dev.ring_inv_or_zero(x, num, out=out)
        assert rep.n_zero == 0 and rep.clean, rep

    def strided():
        rep = dev.is_zero_fill(asg, count)
        assert rep.n_zero == 0 and rep.clean, rep

    cases = {"rs_ring_inv, clean": (ring_inv, 16), "inv_or_zero, clean": (clean, 16), "inv_or_zero, half of the slots zero": (half_zero, 16),
             "inv_or_zero, with a numerator": (with_num, 24), "inv_or_zero, stride 3 in place": (strided, 16)}
    times = {k: [] for k in cases}
    for r in range(WARM + REPEATS):
        for k, (f, _) in cases.items():
            dev.sync()
            t0 = time.perf_counter()
            f()
            dev.sync()
            if r >= WARM:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (times[k], cases[k][1]) for k in cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "inv_or_zero.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("# tools/inv_or_zero_time.py on %s; library sources %s; whole calls, host clock, %d warm-up, median of %d (min, max)"
        % (torch.cuda.get_device_name(0), _lib.source_hash(), WARM, REPEATS))
    for name in PRESETS:
        prm = P.preset(name)
        dev = Device(prm)
        say()
        say("## %s: N = %d, L = %d, %s arithmetic" % (name, prm.N, prm.L, "FP64" if max(prm.q + prm.Q) < 1 << 50 else "Montgomery"))
        say("%-40s %6s %10s %22s %8s %9s" % ("call", "count", "MiB out", "ms", "GB/s", "x ring_inv"))
        for count in COUNTS:
            words = count * prm.ring_words
            res = measure(dev, count)
            base = statistics.median(res["rs_ring_inv, clean"][0])
            for k, (t, bpw) in res.items():
                med = statistics.median(t)
                say("%-40s %6d %10.1f %8.3f (%6.3f, %6.3f) %8.0f %9.2f"
                    % (k, count, words * 8 / 2**20, med, min(t), max(t), bpw * words / (med * 1e-3) / 1e9, base / med))
        del dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
