"""The batched assignment solver and satisfaction check (ringsnark_amd/r1cs_batch.h): B <= 8 assignments of one system
solved, and checked, in one pass over the schedule and the matrices.

CPU (-m "not gpu"): the entry points exist and the header declares what _lib binds.
GPU (-m gpu): every member of a solved batch equals the host mirror ringsnark_amd.r1cs.solve (exact Python integers) of its
own inputs and what rs_r1cs_solve writes, word for word, with the launch counts of ONE single call; every report and flag
row of a checked batch equals Device.r1cs_check of that member.  Exact equality everywhere, no tolerance.  The members of a
batch hold different data (different seeds for the given rows), so a mix-up of members is a mismatch; rows of unknown wires
hold 0xFF bytes before every call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests.test_r1cs_solve import FILL, HAND, MODES, hand_systems, mixed_r1cs, ring256, solved, system, with_fill  # noqa: F401

BATCHES = (1, 2, 3, 5, 8)  # every slot count the kernels are built for (2, 4, 8), a ragged fill of each, and the forwarded 1


# ---- members: (assignment with the unknown rows filled with 0xFF, R.solve of it), built once and never written to ---------
@functools.lru_cache(maxsize=None)
def member(name, b):
    """system(name) with the given rows of member b: member 0 is system(name) itself, the others draw other seeds"""
    prm, cs, given, asg = system(name)
    if b == 0:
        return asg, solved(name)
    if name == "mixed":
        rng = np.random.RandomState(5 + 31 * b)
        rows = [np.stack([rng.randint(0, int(p), prm.N).astype(np.uint64) for p in prm.q]) for _ in given]
    else:
        ctx = H.oracle_ctx(prm)
        rows = ctx.random_ring(7 + 100 * b, len(given)) if name.startswith("logreg") else [ctx.random_ring(7 + 100 * b + k) for k in range(len(given))]
    mine = with_fill(cs, prm, given, rows)
    assert not (mine[list(given)] == asg[list(given)]).all()
    exp = R.solve(cs, given, mine, prm.q)
    exp.setflags(write=False)
    return mine, exp


def upload(dev, name, B, order=None):
    return [dev.put(np.array(member(name, b)[0])) for b in (order or range(B))]


def assert_one_pass(stats, mode, info):
    """the launches of a whole batch are those of ONE rs_r1cs_solve call"""
    if not info.n_solved:
        assert stats == (0, 0)
    elif mode == "levels":
        assert stats == (info.n_levels, 0)
    elif mode == "walk":
        assert stats == (0, 1)
    else:
        assert 1 <= sum(stats) <= info.n_levels


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_batched_solver_and_check():
    from ringsnark_amd import _lib
    lib = _lib.load()
    names = {"rs_r1cs_solve_batch", "rs_r1cs_check_batch"}
    assert names == set(_lib.R1CS_BATCH_SIGNATURES) and all(hasattr(lib, n) for n in names)
    assert lib.rs_version() >= 112
    # the header declares what _lib binds for it, no more and no less (comments aside)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ringsnark_amd", "r1cs_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code)) == names


def test_members_hold_different_data():
    for name in ("wide40", "poly20", "logreg4", "mixed"):
        a0, e0 = member(name, 0)
        a1, e1 = member(name, 1)
        given = system(name)[2]
        assert not (a0[list(given)] == a1[list(given)]).all() and not (e0 == e1).all()


# ---- GPU: solve ----------------------------------------------------------------------------------------------------
def solve_batches(dev, dcs, plan, name, sizes, modes=MODES, **kw):
    """every (B, mode): the batch equals the mirror member by member"""
    from ringsnark_amd.device import to_host
    for B in sizes:
        for mode in modes:
            dasgs = upload(dev, name, B)
            stats = dev.r1cs_solve_batch(plan, dasgs, mode=mode, **kw)
            assert_one_pass(stats, mode, plan.info)
            for b, d in enumerate(dasgs):
                got, exp = to_host(d), member(name, b)[1]
                assert (got == exp).all(), (name, B, mode, b, np.argwhere(got != exp)[:4])
            yield B, mode, dasgs


@pytest.mark.gpu
@pytest.mark.parametrize("force_int", [0, 1])
@pytest.mark.parametrize("name", ["wide40", "poly20", "logreg4"])
def test_batched_solve_equals_the_mirror(name, force_int):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    prm, cs, given, _ = system(name)
    with _lib.tuning(force_int_arith=force_int):
        dev = Device(prm)
        dcs = dev.r1cs(cs)
        plan = dev.r1cs_solve_plan(dcs, given)
        assert plan.info.n_unsolved == 0
        for B, mode, dasgs in solve_batches(dev, dcs, plan, name, BATCHES):
            for d in dasgs:
                assert dev.r1cs_check(dcs, d).n_violated == 0


@pytest.mark.gpu
def test_batched_solve_equals_the_single_call_in_one_pass():
    """`mixed` on ring256: 384 slot pairs (one full chunk of 256 and a ragged one), and RS_SOLVE_AUTO uses both kernels"""
    from ringsnark_amd.device import Device, to_host
    name, B = "mixed", 8
    prm, cs, given, _ = system(name)
    assert prm.L * prm.N // 2 == 384
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    for mode in MODES:
        single, single_stats = [], None
        for d in upload(dev, name, B):
            single_stats = dev.r1cs_solve(plan, d, mode=mode)
            single.append(to_host(d))
        dasgs = upload(dev, name, B)
        stats = dev.r1cs_solve_batch(plan, dasgs, mode=mode)
        assert stats == single_stats, mode  # of the whole batch: the launches of ONE single call
        if mode == "auto":
            assert stats.level_launches >= 2 and stats.walk_launches >= 1
        for b, d in enumerate(dasgs):
            got = to_host(d)
            assert got.tobytes() == single[b].tobytes(), (mode, b)
            assert (got == member(name, b)[1]).all(), (mode, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide40@toy49", "wide40@toy50", "poly20@toy50"])
def test_batched_solve_at_the_top_of_the_fp64_range(name):
    from ringsnark_amd.device import Device
    prm, cs, given, _ = system(name)
    assert all(p < 1 << 50 for p in prm.q + prm.Q) and (name.endswith("toy50")) == all(p > 1 << 49 for p in prm.q)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    for B, mode, dasgs in solve_batches(dev, dcs, plan, name, [8]):
        for d in dasgs:
            assert dev.r1cs_check(dcs, d).n_violated == 0


@pytest.mark.gpu
def test_batched_solve_partial_plan_and_hand_built_rules():
    """unsolved rows still hold 0xFF in every member, solved rows equal the mirror"""
    from ringsnark_amd.device import Device, to_host
    dev = Device(P.preset("toy"))
    for name in ("logreg4_partial",) + HAND:
        prm, cs, given, _ = system(name)
        dcs = dev.r1cs(cs)
        plan = dev.r1cs_solve_plan(dcs, given)
        done = [t for _, t in plan.steps()[0]]
        rest = [v for v in range(cs.n_vars) if v not in given and v not in done]
        if name == "logreg4_partial":
            assert (len(done), len(rest)) == (15, 9)
            with pytest.raises(ValueError) as e:
                dev.r1cs_solve_batch(plan, upload(dev, name, 3))
            assert "first unsolved variable 15;" in str(e.value) and "first blocked constraint 13: an unknown wire in a or b" in str(e.value)
        for B, mode, dasgs in solve_batches(dev, dcs, plan, name, [3], allow_partial=True):
            for b, d in enumerate(dasgs):
                got = to_host(d)
                assert (got[rest] == FILL).all() and (got[done] == member(name, b)[1][done]).all(), (name, mode, b)


@pytest.mark.gpu
def test_permuting_the_members_permutes_the_outputs():
    from ringsnark_amd.device import Device, to_host
    name, order = "wide40", [4, 0, 3, 1, 2]
    prm, cs, given, _ = system(name)
    dev = Device(prm)
    plan = dev.r1cs_solve_plan(dev.r1cs(cs), given)
    for mode in MODES:
        dasgs = upload(dev, name, 5, order)
        dev.r1cs_solve_batch(plan, dasgs, mode=mode)
        for b, d in zip(order, dasgs):
            assert (to_host(d) == member(name, b)[1]).all(), (mode, b)


@pytest.mark.gpu
def test_batched_solve_invalid_arguments():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device, to_host
    name = "wide40"
    prm, cs, given, _ = system(name)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    dasgs = upload(dev, name, 3)
    # one allocation of two assignments and a row, for the overlapping pointers
    row_bytes = prm.L * prm.N * 8
    big = dev.ring_empty(2 * cs.n_vars + 1)
    big.fill_(-1)
    big[:cs.n_vars] = dasgs[0]
    before = [to_host(d).copy() for d in dasgs] + [to_host(big).copy()]
    ptr = lambda *p: (C.c_void_p * 9)(*p)
    d0, d1, d2 = (d.data_ptr() for d in dasgs)
    call = lambda B, ptrs, mode=0, h=None, pl=None: dev.lib.rs_r1cs_solve_batch(dev.h if h is None else h, plan.h if pl is None else pl, B,
                                                                               ptrs, mode, None, dev.stream())
    err = lambda: dev.lib.rs_last_error().decode()
    assert call(0, ptr(d0, d1, d2)) == _lib.RS_ERR_INVALID and err() == "batch out of range"
    assert call(9, ptr(*([d0, d1, d2] * 3))) == _lib.RS_ERR_INVALID and err() == "batch out of range"
    assert call(-1, ptr(d0, d1, d2)) == _lib.RS_ERR_INVALID
    assert call(3, ptr(d0, None, d2)) == _lib.RS_ERR_INVALID and err() == "null batch member"
    assert call(3, None) == _lib.RS_ERR_INVALID
    assert call(3, ptr(d0, d1, d0)) == _lib.RS_ERR_INVALID and err() == "batch members overlap"  # the same pointer
    # a pointer one row into another member: the ranges share all rows but one
    assert call(2, ptr(big.data_ptr(), big.data_ptr() + row_bytes)) == _lib.RS_ERR_INVALID and err() == "batch members overlap"
    assert call(2, ptr(big.data_ptr() + row_bytes, big.data_ptr())) == _lib.RS_ERR_INVALID and err() == "batch members overlap"
    assert call(3, ptr(d0, d1, d2), mode=3) == _lib.RS_ERR_INVALID and err() == "unknown solve mode"
    dev2 = Device(prm)
    assert dev2.lib.rs_r1cs_solve_batch(dev2.h, plan.h, 3, ptr(d0, d1, d2), 0, None, dev2.stream()) == _lib.RS_ERR_INVALID
    assert err() == "solve plan of another context"
    assert dev.lib.rs_r1cs_solve_batch(None, plan.h, 3, ptr(d0, d1, d2), 0, None, dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_r1cs_solve_batch(dev.h, None, 3, ptr(d0, d1, d2), 0, None, dev.stream()) == _lib.RS_ERR_INVALID
    dev.sync()
    after = [to_host(d) for d in dasgs] + [to_host(big)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before))  # none of the refused calls wrote anything
    # two members that touch without overlapping are a legal batch
    big[cs.n_vars:2 * cs.n_vars] = dasgs[1]
    assert call(2, ptr(big.data_ptr(), big.data_ptr() + cs.n_vars * row_bytes)) == _lib.RS_OK
    got = to_host(big)
    assert (got[:cs.n_vars] == member(name, 0)[1]).all() and (got[cs.n_vars:2 * cs.n_vars] == member(name, 1)[1]).all()
    assert (got[2 * cs.n_vars] == FILL).all()


# ---- GPU: check ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def satisfied(preset, kind, m, seed):
    prm = ring256() if preset == "ring256" else P.preset(preset)
    cs = R.wide_r1cs(m, prm.q) if kind == "wide" else R.wide_poly_r1cs(m, prm.q, prm.N)
    asg = H.make_assignment(H.oracle_ctx(prm), cs, seed)
    asg.setflags(write=False)
    return prm, cs, asg


def check_members(preset, kind, m, B):
    """member b by b % 3: 0 one word changed -- at another (wire, limb, slot) per member, the first of them in the last slot of
    the last limb, all others in odd slots; 1 satisfied; 2 many rows violated (every second wire, one slot).  Every member
    starts from an assignment of its own seed."""
    out = []
    for b in range(B):
        prm, cs, asg = satisfied(preset, kind, m, 7 + 10 * b)
        a = asg.copy()
        L, N, nv = prm.L, prm.N, cs.n_vars
        bump = lambda w, l, s: a.__setitem__((w, l, s), (int(a[w, l, s]) + 1) % int(prm.q[l]))
        if b % 3 == 0:
            k = b // 3
            w, l, s = [(nv - 1, L - 1, N - 1), (nv // 2, 0, 7), (1, L - 1, N - 3)][k]
            bump(w, l, s)
        elif b % 3 == 2:
            for w in range(0, nv, 2):
                bump(w, b % L, 2 + b)
        out.append(a)
    return out


def fields(r):
    return tuple(int(getattr(r, f)) for f in ("n_violated", "first_row", "first_limb", "first_slot", "a", "b", "c"))


def assert_batch_check_equals_single(dev, dcs, members, m):
    dasgs = [dev.put(a) for a in members]
    single = [dev.r1cs_check(dcs, d, want_flags=True) for d in dasgs]
    got = dev.r1cs_check_batch(dcs, dasgs, want_flags=True)
    assert len(got) == len(members)
    for b, (g, s) in enumerate(zip(got, single)):
        assert fields(g) == fields(s) and g.satisfied == s.satisfied, (b, fields(g), fields(s))
        gf, sf = g.flags.cpu().numpy(), s.flags.cpu().numpy()
        assert gf.shape == (m,) and gf.dtype == np.uint8 and (gf == sf).all(), (b, np.nonzero(gf)[0][:8], np.nonzero(sf)[0][:8])
        assert int(gf.sum()) == g.n_violated
        if b % 3 == 1:  # the satisfied member between two violated ones
            assert fields(g) == (0, m, 0, 0, 0, 0, 0) and g.satisfied and not gf.any(), b
        else:
            assert g.n_violated >= 1 and not g.satisfied, b
            if b % 3 == 2 and m >= 33:
                assert g.n_violated > 8, b
    # without flag rows of the caller's the reports are the same
    assert [fields(r) for r in dev.r1cs_check_batch(dcs, dasgs)] == [fields(s) for s in single]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 33, 1000])
@pytest.mark.parametrize("preset", ["toy", "toy50", "toy54", "toy60"])
def test_batched_check_equals_the_single_check(preset, m):
    from ringsnark_amd.device import Device
    prm, cs, _ = satisfied(preset, "wide", m, 7)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    for B in (1, 3, 8):
        got = assert_batch_check_equals_single(dev, dcs, check_members(preset, "wide", m, B), m)
        # member 0: its one changed word is the last wire's, in the last slot of the last limb; only the last row reads it
        assert (got[0].n_violated, got[0].first_row, got[0].first_limb, got[0].first_slot) == (1, m - 1, prm.L - 1, prm.N - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,kind,m", [("ring256", "wide", 40), ("toy", "poly", 20), ("toy54", "poly", 20)])
def test_batched_check_slot_chunks_and_polynomial_coefficients(preset, kind, m):
    """ring256: 384 slot pairs, one full chunk of 256 and a ragged one; poly20: coefficients that are ring elements"""
    from ringsnark_amd.device import Device
    prm, cs, _ = satisfied(preset, kind, m, 7)
    dev = Device(prm)
    assert_batch_check_equals_single(dev, dev.r1cs(cs), check_members(preset, kind, m, 5), m)


@pytest.mark.gpu
def test_batched_check_members_may_alias_and_invalid_arguments():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    prm, cs, asg = satisfied("toy", "wide", 33, 7)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    bad = check_members("toy", "wide", 33, 1)[0]
    d_ok, d_bad = dev.put(np.array(asg)), dev.put(bad)  # a copy: the shared assignments are read-only
    got = dev.r1cs_check_batch(dcs, [d_ok, d_bad, d_ok, d_bad])
    one = dev.r1cs_check(dcs, d_bad)
    assert [fields(g) for g in got] == [(0, 33, 0, 0, 0, 0, 0), fields(one)] * 2
    reps = (_lib.R1csReport * 9)()
    ptrs = (C.c_void_p * 9)(*([d_ok.data_ptr()] * 9))
    call = lambda B, p=ptrs, r=reps: dev.lib.rs_r1cs_check_batch(dev.h, dcs.h, B, p, None, r, dev.stream())
    assert call(0) == _lib.RS_ERR_INVALID and call(9) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_last_error().decode() == "batch out of range"
    assert call(2, (C.c_void_p * 9)(d_ok.data_ptr(), None)) == _lib.RS_ERR_INVALID
    assert call(2, None) == _lib.RS_ERR_INVALID and call(2, ptrs, None) == _lib.RS_ERR_INVALID
