"""The assignment solver (ringsnark_amd/r1cs_solve.h) beside the bespoke ways to build an assignment, in one session on one
machine.  Per shape: plan-build ms (rs_r1cs_solve_plan_create: the host schedule, O(nnz), and the upload of its arrays), and
per mode (auto, levels, walk) the launches and the solve ms (median of 5 after one warm-up, wall clock around a synchronised
call), then the bespoke path of the same assignment where there is one:
  chain    chain_r1cs at 2^16 on C3            rs_chain_assignment (one kernel, the two operands carried in registers)
  logreg   logreg_r1cs(256) on C5 and on C3    ringsnark_amd.r1cs.logreg_assignment on the Device ring operations
  wide     wide_r1cs at 2^13 on C3             none on the device
Every solved assignment is compared with the bespoke one word for word where there is one, and checked with rs_r1cs_check.

Every shape runs in a process of its own under `timeout -k 10`, one after another, and the first that fails ends the run.
usage: tools/r1cs_solve_time.py [--out FILE] [--small]    (default profiles/r1cs_solve.txt; --small: toy-sized shapes, a dry run)"""
import argparse
import statistics
import subprocess
import sys
import time

CASES = ("chain:C3", "logreg:C5", "logreg:C3", "wide:C3")
CASE_SECONDS = 240


def driver(a):
    open(a.out, "w").write("")
    for case in CASES:  # chained: a shape that fails (or runs into its time limit) ends the run
        cmd = ["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, sys.argv[0], "--out", a.out, "--case", case] + (["--small"] if a.small else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("case %s ended with status %d: stopping" % (case, rc), flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r1cs_solve.txt")
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    if a.case is None:
        sys.exit(driver(a))

    import torch

    sys.path.insert(0, ".")
    from ringsnark_amd import params as P
    from ringsnark_amd import r1cs as R
    from ringsnark_amd.device import Device

    def say(s):
        print(s, flush=True)
        open(a.out, "a").write(s + "\n")

    kind, preset = a.case.split(":")
    prm = P.preset("toy" if a.small else preset)
    dev = Device(prm)
    if a.case == CASES[0]:
        say("# tools/r1cs_solve_time.py%s: ms, median of 5 after one warm-up, wall clock around a synchronised call" % (" --small" if a.small else ""))

    def timed(fn, reps=5):
        ts = []
        for s in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.time()
            out = fn()
            torch.cuda.synchronize()
            if s:
                ts.append((time.time() - t0) * 1e3)
        return statistics.median(ts), out

    bespoke = None
    if kind == "chain":
        m = 1 << (8 if a.small else 16)
        cs, n_given, name = R.chain_r1cs(m, prm.q), 2, "chain_r1cs(2^%d)" % (m.bit_length() - 1)
        base = dev.ring_empty(cs.n_vars)
        base.fill_(-1)
        dev.fill_uniform(base[:2], 0, 9)
        exp = base.clone()
        bespoke = ("rs_chain_assignment", lambda: dev.chain_assignment(exp, m))
    elif kind == "logreg":
        F = 8 if a.small else 256
        cs, n_given, name = R.logreg_r1cs(prm.q, F), 4 * F, "logreg_r1cs(%d)" % F
        inputs = dev.fill_uniform(dev.ring_empty(4 * F), 0, 41)
        base = dev.ring_empty(cs.n_vars)
        base.fill_(-1)
        base[:4 * F] = inputs
        bespoke = ("logreg_assignment on Device ring operations", lambda: R.logreg_assignment(F, inputs, dev.ring_mul, dev.ring_add, dev.ring_mul_scalar))
    else:
        m = 1 << (8 if a.small else 13)
        cs, n_given, name = R.wide_r1cs(m, prm.q), 2, "wide_r1cs(2^%d)" % (m.bit_length() - 1)
        base = dev.ring_empty(cs.n_vars)
        base.fill_(-1)
        dev.fill_uniform(base[:2], 0, 9)
    dcs = dev.r1cs(cs)
    t0 = time.time()
    plan = dev.r1cs_solve_plan(dcs, range(n_given))
    t_plan = (time.time() - t0) * 1e3
    i = plan.info
    say("%s on %s (N = %d, L = %d): %d constraints, %d variables, %d given, %d solved in %d levels (widest %d); plan build %.1f ms"
        % (name, prm.name, prm.N, prm.L, cs.m, cs.n_vars, i.n_given, i.n_solved, i.n_levels, i.max_width, t_plan))
    assert i.n_unsolved == 0
    want = None
    if bespoke:
        t, want = timed(bespoke[1])
        say("    %-44s %9.3f ms" % (bespoke[0], t))
    got = base.clone()
    for mode in ("auto", "levels", "walk"):
        got.copy_(base)
        t, stats = timed(lambda: dev.r1cs_solve(plan, got, mode=mode))
        assert dev.r1cs_check(dcs, got).satisfied, mode
        if want is not None:
            assert torch.equal(got, want), mode
        say("    %-44s %9.3f ms   (%d level launches, %d walk launches)" % ("rs_r1cs_solve, " + mode, t, stats.level_launches, stats.walk_launches))


if __name__ == "__main__":
    main()
