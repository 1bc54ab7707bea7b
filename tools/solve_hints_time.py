"""Solver hints (ringsnark_amd/solve_hints.h) against the staged flow a caller writes from the entry points that existed
before them, on one MI355X at the C3 ring (N = 8192, L = 4).

  circuits   running_max_r1cs(nbits = 16, count = 64): 192 levels that alternate constraint, BITS hint, constraint;
             continued_fraction_r1cs(count = 1024): 2048 levels that alternate constraint, QUOT hint, all slot-local.
  hinted     one rs_r1cs_hint_plan_create, then rs_r1cs_solve_hinted in each mode (enqueue only, no report).
  staged     the parent's code: rs_r1cs_solve_plan_create from the wires known so far, rs_r1cs_solve (auto), then the fills
             (rs_ring_bit_decompose / rs_ring_inv_or_zero, enqueue only) of the hints whose sources are now known, marked as
             given for the next plan -- once per dependent stage.  Its plan builds are timed apart: they are once per system.
Wall clock around a synchronised call; one warm-up, then the median of 5 (min and max beside it).  Both flows must leave the
same words, and rs_r1cs_check must accept them.

usage: python tools/solve_hints_time.py [--out profiles/solve_hints.txt] [--preset C3] [--max-count 64] [--cf-count 1024]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402
from ringsnark_amd.device import Device  # noqa: E402

REPEATS, WARM = 5, 1
NBITS = 16


def spread(t):
    return "%.3f ms (min %.3f, max %.3f)" % (statistics.median(t), min(t), max(t))


def host_time(dev, f, setup=lambda: None):
    t = []
    for k in range(WARM + REPEATS):
        setup()
        dev.sync()
        t0 = time.perf_counter()
        f()
        dev.sync()
        if k >= WARM:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


def staged_plans(dev, dcs, given, hints):
    """The staged flow's schedule: [(plan, [hints to fill after it])], built from the wires known so far, stage by stage."""
    cs = dcs.cs
    known = R.given_mask(cs, given).astype(bool)
    todo, stages = list(hints), []
    while True:
        plan = dev.r1cs_solve_plan(dcs, known)
        for _, w in plan.steps()[0]:
            known[w] = True
        ready = [h for h in todo if all(known[v] for v in h.sources)]
        stages.append((plan, ready))
        if not ready:
            return stages
        for h in ready:
            known[h.targets] = True
        todo = [h for h in todo if h not in ready]


def staged_run(dev, stages, asg):
    rows = asg.view(-1, dev.L, dev.N)
    for plan, fills in stages:
        if plan.info.n_solved:
            dev.r1cs_solve(plan, asg, allow_partial=True)
        for h in fills:
            if h.kind == R.RS_HINT_BITS:
                assert h.dst_stride == 1, "the stand-alone fill writes consecutive bit rows"
                dev.ring_bit_decompose(rows[h.src:h.src + 1], h.nbits, out=rows[h.dst:h.dst + h.nbits], want_report=False)
            else:
                num = rows[h.num:h.num + 1] if h.kind == R.RS_HINT_QUOT else None
                dev.ring_inv_or_zero(rows[h.src:h.src + 1], num=num, out=rows[h.dst:h.dst + 1], want_report=False)


def measure(dev, name, cs, hints, given, inputs, lines):
    dcs = dev.r1cs(cs)
    fresh = torch.full((cs.n_vars, dev.L, dev.N), 0x25A5A5A5A5A5A5A5, dtype=torch.int64, device=dev.device)
    fresh[: inputs.shape[0]] = inputs
    asg = fresh.clone()
    reset = lambda: asg.copy_(fresh)
    lines.append("%s: m = %d, n_vars = %d, %d hints, assignment %.0f MiB" % (name, cs.m, cs.n_vars, len(hints), asg.numel() * 8 / 2**20))
    t = []
    for _ in range(WARM + REPEATS):
        t0 = time.perf_counter()
        plan = dev.r1cs_hint_plan(dcs, given, hints)
        t.append((time.perf_counter() - t0) * 1e3)
    assert plan.info.n_unsolved == 0
    lines.append("  hinted plan create (%d levels, %d steps)            %s" % (plan.info.n_levels, plan.info.n_steps, spread(t[WARM:])))
    results = {}
    for mode in ("auto", "levels", "walk"):
        stats = dev.r1cs_solve_hinted(plan, asg, mode=mode, want_report=False)[0]
        t = host_time(dev, lambda: dev.r1cs_solve_hinted(plan, asg, mode=mode, want_report=False), reset)
        results[mode] = asg.clone() if mode == "auto" else None
        if mode != "auto":
            assert torch.equal(asg, results["auto"]), "modes differ"
        lines.append("  hinted solve, %-6s (%4d level, %4d walk, %4d hint launches)  %s" % (mode, stats[0], stats[1], stats[2], spread(t)))
    assert dev.r1cs_check(dcs, results["auto"]).satisfied
    t0 = time.perf_counter()
    stages = staged_plans(dev, dcs, given, hints)
    build = (time.perf_counter() - t0) * 1e3
    t = host_time(dev, lambda: staged_run(dev, stages, asg), reset)
    assert torch.equal(asg, results["auto"]), "the staged flow leaves other words"
    lines.append("  staged flow, %d plans built once                     %.1f ms" % (len(stages), build))
    lines.append("  staged flow, %d solves and %d fills                  %s" % (sum(1 for p, _ in stages if p.info.n_solved),
                                                                               sum(len(f) for _, f in stages), spread(t)))
    for p, _ in stages:
        p.close()
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--preset", default="C3")
    ap.add_argument("--max-count", type=int, default=64)
    ap.add_argument("--cf-count", type=int, default=1024)
    args = ap.parse_args()
    prm = P.preset(args.preset)
    dev = Device(prm)
    gen = torch.Generator(device=dev.device).manual_seed(7)
    lines = ["solver hints against the staged flow, %s (N = %d, L = %d), %s" % (args.preset, prm.N, prm.L, torch.cuda.get_device_name(0))]
    cs, hints = R.running_max_r1cs(prm.q, NBITS, args.max_count)
    x = torch.randint(0, 1 << (NBITS - 1), (args.max_count + 1, 1, prm.N), generator=gen, device=dev.device, dtype=torch.int64)
    inputs = torch.cat([torch.ones((1, prm.L, prm.N), dtype=torch.int64, device=dev.device), x.expand(-1, prm.L, -1)])
    measure(dev, "running_max_r1cs(nbits = %d, count = %d)" % (NBITS, args.max_count), cs, hints, range(args.max_count + 2), inputs, lines)
    cs, hints = R.continued_fraction_r1cs(prm.q, args.cf_count)
    r = torch.randint(1, 1 << 30, (1 + 2 * args.cf_count, prm.L, prm.N), generator=gen, device=dev.device, dtype=torch.int64)
    inputs = torch.cat([torch.ones((1, prm.L, prm.N), dtype=torch.int64, device=dev.device), r])
    measure(dev, "continued_fraction_r1cs(count = %d)" % args.cf_count, cs, hints, range(2 + 2 * args.cf_count), inputs, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
