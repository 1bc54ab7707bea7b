"""The batched assignment solver and satisfaction check (ringsnark_amd/r1cs_batch.h) beside B calls of the single entry
points, in one session on one machine, on the four shapes of tools/r1cs_solve_time.py:
  chain    chain_r1cs at 2^16 on C3
  logreg   logreg_r1cs(256) on C5 and on C3
  wide     wide_r1cs at 2^13 on C3
Per shape and B in {1, 2, 4, 8}: B members with different given rows; rs_r1cs_solve_batch (one call) against B calls of
rs_r1cs_solve under RS_SOLVE_AUTO (the logreg shapes also under RS_SOLVE_LEVELS), and rs_r1cs_check_batch against B calls of
rs_r1cs_check on the solved members.  Both sides are warmed up once, then alternate in one process; ms per MEMBER, median of 5
with min and max, wall clock around calls that end in a synchronise.  Before any timing the batched outputs are compared with
the single ones word for word (solve) and field for field (check).  A shape whose B members and one reference copy do not fit
in 80 % of the free device memory is timed up to the largest B that does, and says so.

Every shape runs in a process of its own under `timeout -k 10`, one after another, and the first that fails ends the run.
usage: tools/r1cs_batch_time.py [--out FILE] [--small]    (default profiles/r1cs_batch.txt; --small: toy-sized shapes, a dry run)"""
import argparse
import statistics
import subprocess
import sys
import time

CASES = ("chain:C3", "logreg:C5", "logreg:C3", "wide:C3")
BATCHES = (1, 2, 4, 8)
CASE_SECONDS = 300
REPS = 5


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
    ap.add_argument("--out", default="profiles/r1cs_batch.txt")
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
        say("# tools/r1cs_batch_time.py%s: ms per member, median of %d (min .. max) after one warm-up of both sides, the two sides alternating;"
            % (" --small" if a.small else "", REPS))
        say("# wall clock around calls that end in a synchronise; ratio = batched / single per member (below 1: the batch is faster)")

    if kind == "chain":
        m = 1 << (8 if a.small else 16)
        cs, n_given, name = R.chain_r1cs(m, prm.q), 2, "chain_r1cs(2^%d)" % (m.bit_length() - 1)
    elif kind == "logreg":
        F = 8 if a.small else 256
        cs, n_given, name = R.logreg_r1cs(prm.q, F), 4 * F, "logreg_r1cs(%d)" % F
    else:
        m = 1 << (8 if a.small else 13)
        cs, n_given, name = R.wide_r1cs(m, prm.q), 2, "wide_r1cs(2^%d)" % (m.bit_length() - 1)
    modes = ("auto", "levels") if kind == "logreg" else ("auto",)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, range(n_given))
    i = plan.info
    assert i.n_unsolved == 0
    member_bytes = cs.n_vars * prm.L * prm.N * 8
    free = torch.cuda.mem_get_info()[0]
    fits = [B for B in BATCHES if (B + 1) * member_bytes <= 0.8 * free]
    say("%s on %s (N = %d, L = %d): %d constraints, %d variables, %d given, %d solved in %d levels (widest %d); %.2f GiB per member"
        % (name, prm.name, prm.N, prm.L, cs.m, cs.n_vars, i.n_given, i.n_solved, i.n_levels, i.max_width, member_bytes / 2.0**30))
    if len(fits) < len(BATCHES):
        say("    %.1f GiB free on the device: B members and one reference copy fit up to B = %d" % (free / 2.0**30, fits[-1]))

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(single, batched, B):
        single(), batched()  # warm-up of both sides
        ts, tb = [], []
        for _ in range(REPS):
            ts.append(clock(single) / B)
            tb.append(clock(batched) / B)
        return ts, tb

    def row(label, B, ts, tb, extra=""):
        ms, mb = statistics.median(ts), statistics.median(tb)
        say("    %-22s B = %d   single %9.3f (%9.3f .. %9.3f)   batched %9.3f (%9.3f .. %9.3f)   ratio %5.2f%s"
            % (label, B, ms, min(ts), max(ts), mb, min(tb), max(tb), mb / ms, extra))

    members = []
    for B in fits:
        while len(members) < B:  # member b: its own given rows, 0xFF bytes everywhere else
            t = dev.ring_empty(cs.n_vars)
            t.fill_(-1)
            dev.fill_uniform(t[:n_given], 0, 9 + 50 * len(members))
            members.append(t)
        batch = members[:B]

        def reset():
            for t in batch:
                t[n_given:].fill_(-1)

        for mode in modes:
            # word for word before any timing: every member solved alone (into the reference copy) against the batch
            reset()
            stats_b = dev.r1cs_solve_batch(plan, batch, mode=mode)
            ref = dev.ring_empty(cs.n_vars)
            for t in batch:
                ref.fill_(-1)
                ref[:n_given] = t[:n_given]
                stats_s = dev.r1cs_solve(plan, ref, mode=mode)
                assert torch.equal(ref, t), (mode, B)
            assert stats_b == stats_s, (stats_b, stats_s)
            del ref
            ts, tb = alternate(lambda: [dev.r1cs_solve(plan, t, mode=mode) for t in batch], lambda: dev.r1cs_solve_batch(plan, batch, mode=mode), B)
            row("solve, " + mode, B, ts, tb, "   (%d level + %d walk launches per call)" % stats_b)
        # the check, on the solved members and with one word of the last member changed
        last = batch[-1]
        word = last[cs.n_vars - 1, prm.L - 1, prm.N - 1].clone()
        for tamper in (False, True):
            if tamper:
                last[cs.n_vars - 1, prm.L - 1, prm.N - 1] = (word + 1) % prm.q[prm.L - 1]
            single = [dev.r1cs_check(dcs, t) for t in batch]
            got = dev.r1cs_check_batch(dcs, batch)
            assert got == single, B  # R1csCheck: every field
            assert all(s.satisfied for s in single[:-1]) and single[-1].satisfied == (not tamper)
        last[cs.n_vars - 1, prm.L - 1, prm.N - 1] = word
        ts, tb = alternate(lambda: [dev.r1cs_check(dcs, t) for t in batch], lambda: dev.r1cs_check_batch(dcs, batch), B)
        row("check", B, ts, tb)


if __name__ == "__main__":
    main()
