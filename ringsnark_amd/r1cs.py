"""Host-side R1CS container in CSR form + the synthetic circuits of SURVEY.md section 8(d).

Mirrors what the hot path reads from the reference's r1cs_constraint_system<RingT>
(relations/constraint_satisfaction_problems/r1cs/r1cs.hpp:118-123): for every constraint i the
three linear combinations a, b, c as lists of (index, coeff) with index 0 = the constant one
(relations/variable.tcc:246-254).  A coefficient is a RingT: either a slot-constant ring scalar, stored
reduced per RNS limb as uint64[L][nnz] (a signed literal c < 0 is -c's negation mod q_i, i.e.
-RingT::one()*|c|), or a general ring element (one residue per NTT slot: the DFT
constraint of benchmarks/bench_ntt_SEAL.cpp:46-53 multiplies variables by powers of a polynomial), kept
once in `poly_table` [n_poly][L][N] and referenced per non-zero by `poly_idx` (-1 = the scalar).
"""
import collections
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np


@dataclass
class R1CS:
    m: int  # constraints
    n_vars: int  # variables, excluding the constant one
    n_inputs: int  # primary inputs (the first n_inputs variables)
    mats: Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray]]  # a/b/c -> (row_ptr, col, coeff[L][nnz])
    poly_idx: Optional[Dict[str, np.ndarray]] = None  # a/b/c -> int32[nnz], -1 = scalar coefficient of mats
    poly_table: Optional[np.ndarray] = None  # uint64 [n_poly][L][N]: coefficients that are general ring elements

    @property
    def n_aux(self):
        return self.n_vars - self.n_inputs

    def nnz(self, name):
        return int(self.mats[name][1].shape[0])


def from_rows(m, n_vars, n_inputs, rows: Dict[str, List[List[Tuple[int, object]]]], q: List[int]) -> R1CS:
    """rows[name][i] = [(index, coeff), ...]; coeff: a signed int (slot-constant scalar) or a uint64 array [L][N]
    (a general ring element)."""
    mats, pidx, table = {}, {}, []
    for name in "abc":
        rp = np.zeros(m + 1, dtype=np.uint32)
        col, cf, pi = [], [], []
        for i, terms in enumerate(rows[name]):
            for idx, c in terms:
                assert 0 <= idx <= n_vars
                col.append(idx)
                if isinstance(c, np.ndarray):
                    assert c.ndim == 2 and c.shape[0] == len(q)
                    pi.append(len(table))
                    table.append(np.ascontiguousarray(c, dtype=np.uint64))
                    cf.append(0)
                else:
                    pi.append(-1)
                    cf.append(c)
            rp[i + 1] = len(col)
        coeff = np.array([[c % p for c in cf] for p in q], dtype=np.uint64).reshape(len(q), len(cf))
        mats[name] = (rp, np.array(col, dtype=np.uint32), coeff)
        pidx[name] = np.array(pi, dtype=np.int32)
    if not table:
        return R1CS(m, n_vars, n_inputs, mats)
    return R1CS(m, n_vars, n_inputs, mats, pidx, np.stack(table))


@dataclass
class R1csCheck:
    """What a satisfaction check reports (rs_r1cs_report of ringsnark_amd/r1cs_check.h, field for field)."""
    n_violated: int  # constraints violated in at least one (limb, slot)
    first_row: int  # lowest violated constraint; m when there is none
    first_limb: int  # with first_slot: the lowest ring-layout index limb*N + slot that violates first_row
    first_slot: int
    a: int  # canonical residues of the three evaluations there; 0 when there is none
    b: int
    c: int
    flags: object = None  # uint8 [m], 1 = violated (numpy on the host, a torch tensor from the device), or None

    @property
    def satisfied(self):
        return self.n_violated == 0


def is_satisfied(cs: R1CS, assignment, q: List[int]) -> R1csCheck:
    """r1cs_constraint_system::is_satisfied (relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:122-158) on the
    host, exact (Python integers): <a,(1,x)> * <b,(1,x)> == <c,(1,x)> for every constraint, limb and slot, and where it
    first fails.  assignment: [n_vars][L][N] canonical residues (all n_vars rows).  The host mirror of the device check."""
    asg = np.asarray(assignment)
    L = len(q)
    assert asg.ndim == 3 and asg.shape[0] == cs.n_vars and asg.shape[1] == L, asg.shape
    N = asg.shape[2]
    x = asg.astype(object)
    ev = np.zeros((3, cs.m, L, N), dtype=object)
    for k, name in enumerate("abc"):
        rp, col, coeff = cs.mats[name]
        pidx = None if cs.poly_idx is None else cs.poly_idx[name]
        for i in range(cs.m):
            for e in range(int(rp[i]), int(rp[i + 1])):
                for l in range(L):
                    if pidx is not None and pidx[e] >= 0:
                        cf = cs.poly_table[int(pidx[e]), l].astype(object)
                    else:
                        cf = int(coeff[l, e])
                    v = 1 if col[e] == 0 else x[int(col[e]) - 1, l]
                    ev[k, i, l] = (ev[k, i, l] + cf * v) % int(q[l])
    qs = np.array([int(p) for p in q], dtype=object).reshape(1, L, 1)
    bad = ((ev[0] * ev[1]) % qs != ev[2]).reshape(cs.m, L * N)
    flags = bad.any(axis=1).astype(np.uint8)
    n = int(flags.sum())
    if n == 0:
        return R1csCheck(0, cs.m, 0, 0, 0, 0, 0, flags)
    row = int(np.argmax(flags))
    idx = int(np.argmax(bad[row]))
    limb, slot = idx // N, idx % N
    return R1csCheck(n, row, limb, slot, int(ev[0, row, limb, slot]), int(ev[1, row, limb, slot]), int(ev[2, row, limb, slot]), flags)


@dataclass
class SolveInfo:
    """What a solve plan reports (rs_r1cs_solve_info of ringsnark_amd/r1cs_solve.h, field for field)."""
    n_given: int
    n_solved: int
    n_unsolved: int
    first_unsolved: int  # lowest 0-based variable neither given nor solved; n_vars when there is none
    n_levels: int
    max_width: int
    n_unused: int  # constraints that determine nothing (checks, or never ready)
    first_blocked: int  # lowest constraint never ready that still holds an unknown wire; m when there is none
    blocked_reason: int  # of first_blocked, a key of SOLVE_BLOCKED


# csrc/r1cs_solve.hip: RS_SOLVE_AUTO gives a level to the level kernel when width * slot chunks (of 256 slot pairs) reaches this
SOLVE_FILL_WORKGROUPS = 256
SOLVE_BLOCKED = {0: "nothing is blocked", 1: "an unknown wire in a or b", 2: "several unknown wires in c",
                 3: "a polynomial coefficient on the target", 4: "the target's coefficients sum to 0 modulo a ring prime",
                 5: "the target also occurs in a or b"}


def given_mask(cs: R1CS, given) -> np.ndarray:
    """uint8 [n_vars] from a bool mask of that length or from an iterable of 0-based variables."""
    g = np.asarray(list(given) if not isinstance(given, np.ndarray) else given)
    if g.dtype == np.bool_:
        assert g.shape == (cs.n_vars,), g.shape
        return g.astype(np.uint8)
    mask = np.zeros(cs.n_vars, dtype=np.uint8)
    idx = g.astype(np.int64)
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < cs.n_vars), "given variable out of range"
    mask[idx] = 1
    return mask


def solve_schedule(cs: R1CS, given, q: List[int]):
    """The schedule of the assignment solver (ringsnark_amd/r1cs_solve.h), the host mirror of rs_r1cs_solve_plan_create.
    Variables are 0-based (variable v is column v + 1; column 0 is the constant one).  Constraint j is ready when every wire
    of a and b is known, c holds exactly one distinct unknown wire w, every c entry on w has a scalar coefficient and their
    sum is non-zero modulo every q_l.  Given wires have level 0, a step's level is 1 + the highest level among the wires
    its constraint reads, a wire is determined in the lowest level in which a constraint for it is ready and there by the
    lowest such constraint; steps are ordered by (level, constraint).  Unknown-counters per constraint and a wire ->
    constraint adjacency: O(nnz) apart from sorting each level.  One scheduler body: solve_hinted_schedule without hints.
    Returns (steps [(constraint, variable)], level_ptr [n_levels + 1], SolveInfo)."""
    steps, level_ptr, info = solve_hinted_schedule(cs, given, (), q)
    return [(j, t) for _, j, t in steps], level_ptr, SolveInfo(*[getattr(info, f.name) for f in dataclasses.fields(SolveInfo)])


RS_HINT_BITS, RS_HINT_INV, RS_HINT_QUOT = 1, 2, 3
SOLVE_BLOCKED[6] = "the only unknown is reserved for a hint that never became ready"


@dataclass(frozen=True)
class Hint:
    """A declared hint (rs_solve_hint of ringsnark_amd/solve_hints.h, field for field; 0-based variables).
    BITS: variable dst + k * dst_stride <- bit k of src, k < nbits.  INV: dst <- src^-1, 0 where src is 0.
    QUOT: dst <- num * src^-1, 0 where src is 0."""
    kind: int
    src: int
    num: int
    dst: int
    nbits: int = 0
    dst_stride: int = 1

    @staticmethod
    def bits(src, dst, nbits, dst_stride=1):
        return Hint(RS_HINT_BITS, src, 0, dst, nbits, dst_stride)

    @staticmethod
    def inv(src, dst):
        return Hint(RS_HINT_INV, src, 0, dst)

    @staticmethod
    def quot(num, src, dst):
        return Hint(RS_HINT_QUOT, src, num, dst)

    @property
    def targets(self):
        return [self.dst + k * self.dst_stride for k in range(self.nbits)] if self.kind == RS_HINT_BITS else [self.dst]

    @property
    def sources(self):
        return [self.src, self.num] if self.kind == RS_HINT_QUOT and self.num != self.src else [self.src]


@dataclass
class HintSolveInfo(SolveInfo):
    """What a hint plan reports (rs_r1cs_hint_info of ringsnark_amd/solve_hints.h): the fields of SolveInfo -- n_solved counts
    wires, from constraints and hints alike; max_width counts the steps of a level -- and those of the hints."""
    n_steps: int = 0
    n_hints_run: int = 0
    n_hints_blocked: int = 0
    first_blocked_hint: int = 0  # lowest hint that never became ready; the number of hints when there is none


def check_hints(cs: R1CS, given, hints, q: List[int]):
    """The refusals of rs_r1cs_hint_plan_create (ValueError), in its order."""
    known = given_mask(cs, given).astype(bool)
    nv, taken = cs.n_vars, set()
    for i, h in enumerate(hints):
        if h.kind not in (RS_HINT_BITS, RS_HINT_INV, RS_HINT_QUOT):
            raise ValueError("hint %d: unknown kind" % i)
        if not (0 <= h.src < nv and 0 <= h.dst < nv and (h.kind != RS_HINT_QUOT or 0 <= h.num < nv)):
            raise ValueError("hint %d: variable out of range" % i)
        if h.kind == RS_HINT_BITS:
            if not 1 <= h.nbits <= max_nbits(q):
                raise ValueError("hint %d: nbits must be between 1 and min_i floor(log2 q_i) = %d" % (i, max_nbits(q)))
            if h.dst_stride < 1:
                raise ValueError("hint %d: dst_stride must be at least 1" % i)
            if h.dst + (h.nbits - 1) * h.dst_stride >= nv:
                raise ValueError("hint %d: variable out of range" % i)
        for v in h.targets:
            if known[v]:
                raise ValueError("hint %d: target %d is given" % (i, v))
            if v in taken:
                raise ValueError("hint %d: target %d is named twice" % (i, v))
            if v in h.sources:
                raise ValueError("hint %d: a source is among its own targets" % i)
            taken.add(v)


def solve_hinted_schedule(cs: R1CS, given, hints, q: List[int]):
    """The schedule of the solver with hints (ringsnark_amd/solve_hints.h), the host mirror of rs_r1cs_hint_plan_create: the
    rules of solve_schedule, and: the targets of every hint are reserved (no constraint step determines one; for the constraint
    counters they are unknown until their hint has run); a hint is ready when its sources are known, its level is 1 + the
    highest level of its sources; steps are ordered by level, then constraint steps by row, then hint steps by hint index.
    Hints that never become ready (a cycle across hints, an unknown source) are reported, not refused.
    Returns (steps [(kind, index, wire)] -- kind 0: constraint and target, kind 1: hint and its first target --,
    level_ptr [n_levels + 1], HintSolveInfo)."""
    hints = list(hints)
    check_hints(cs, given, hints, q)
    m, nv = cs.m, cs.n_vars
    known = given_mask(cs, given).astype(bool)
    n_given = int(known.sum())
    rp = {n: [int(x) for x in cs.mats[n][0]] for n in "abc"}
    col = {n: [int(x) for x in cs.mats[n][1]] for n in "abc"}
    unk_ab, unk_c = [set() for _ in range(m)], [set() for _ in range(m)]
    adj = [[] for _ in range(nv)]  # wire -> (constraint, in c)
    for j in range(m):
        for n in "abc":
            side = unk_c[j] if n == "c" else unk_ab[j]
            for e in range(rp[n][j], rp[n][j + 1]):
                v = col[n][e] - 1
                if v >= 0 and not known[v] and v not in side:
                    side.add(v)
                    adj[v].append((j, n == "c"))
    reserved = {v for h in hints for v in h.targets}
    unk_h = [{v for v in h.sources if not known[v]} for h in hints]
    hadj = collections.defaultdict(list)  # wire -> hints that read it
    for i, srcs in enumerate(unk_h):
        for v in srcs:
            hadj[v].append(i)
    hint_done = [False] * len(hints)
    candidate = lambda j: not unk_ab[j] and len(unk_c[j]) == 1
    pidx = None if cs.poly_idx is None else cs.poly_idx["c"]
    coeff = cs.mats["c"][2]
    steps, level_ptr, is_step, max_width, n_wires = [], [0], [False] * m, 0, 0
    cand = [j for j in range(m) if candidate(j)]
    hcand = [i for i, srcs in enumerate(unk_h) if not srcs]
    while cand or hcand:
        fresh, width = {}, len(steps)
        for j in sorted(cand):
            if not candidate(j):
                continue
            (t,) = unk_c[j]
            if t in fresh or t in reserved:
                continue  # a lower constraint of this level determines it; its hint determines it, or nothing does
            on_t = [e for e in range(rp["c"][j], rp["c"][j + 1]) if col["c"][e] == t + 1]
            if pidx is not None and any(pidx[e] >= 0 for e in on_t):
                continue
            if any(sum(int(coeff[l, e]) for e in on_t) % int(q[l]) == 0 for l in range(len(q))):
                continue
            fresh[t] = j
            is_step[j] = True
            steps.append((0, j, t))
        for i in sorted(hcand):
            hint_done[i] = True
            steps.append((1, i, hints[i].dst))
            for v in hints[i].targets:
                fresh[v] = None
        if not fresh:
            break
        level_ptr.append(len(steps))
        max_width = max(max_width, len(steps) - width)
        n_wires += len(fresh)
        cand, hcand = [], []
        for t in fresh:
            known[t] = True
        for t in fresh:
            for j, in_c in adj[t]:
                (unk_c if in_c else unk_ab)[j].discard(t)
                if candidate(j):
                    cand.append(j)
            for i in hadj[t]:
                unk_h[i].discard(t)
                if not unk_h[i]:
                    hcand.append(i)
    unsolved = [v for v in range(nv) if not known[v]]
    blocked = [j for j in range(m) if not is_step[j] and (unk_ab[j] or unk_c[j])]
    reason = 0
    if blocked:
        j = blocked[0]
        if len(unk_c[j]) == 1 and unk_ab[j] == unk_c[j]:
            reason = 5
        elif unk_ab[j]:
            reason = 1
        elif len(unk_c[j]) > 1:
            reason = 2
        else:
            (t,) = unk_c[j]
            poly = pidx is not None and any(pidx[e] >= 0 for e in range(rp["c"][j], rp["c"][j + 1]) if col["c"][e] == t + 1)
            reason = 6 if t in reserved else 3 if poly else 4
    n_constraint = sum(1 for s in steps if s[0] == 0)
    n_run = sum(hint_done)
    info = HintSolveInfo(n_given, n_wires, len(unsolved), unsolved[0] if unsolved else nv, len(level_ptr) - 1, max_width,
                         m - n_constraint, blocked[0] if blocked else m, reason, len(steps), n_run, len(hints) - n_run,
                         hint_done.index(False) if n_run < len(hints) else len(hints))
    return steps, level_ptr, info


def _solve_step(cs: R1CS, out, j, t, q):
    """Row t of `out` from constraint j: (<a,(1,x)> * <b,(1,x)> - <c,(1,x)> without t) * k^-1, exact."""
    def row(name, l, skip):
        rp, col, coeff = cs.mats[name]
        pidx = None if cs.poly_idx is None else cs.poly_idx[name]
        acc, k = np.zeros(out.shape[2], dtype=object), 0
        for e in range(int(rp[j]), int(rp[j + 1])):
            if int(col[e]) == skip:
                k += int(coeff[l, e])
                continue
            cf = cs.poly_table[int(pidx[e]), l].astype(object) if pidx is not None and pidx[e] >= 0 else int(coeff[l, e])
            acc = (acc + cf * (1 if col[e] == 0 else out[int(col[e]) - 1, l].astype(object))) % int(q[l])
        return acc, k

    for l in range(len(q)):
        p = int(q[l])
        (a, _), (b, _), (c, k) = row("a", l, -1), row("b", l, -1), row("c", l, t + 1)
        out[t, l] = ((a * b - c) * pow(k % p, -1, p) % p).astype(np.uint64)


def solve(cs: R1CS, given, assignment, q: List[int]) -> np.ndarray:
    """The assignment solver on the host in exact Python integers, the host mirror of rs_r1cs_solve: a copy of `assignment`
    [n_vars][L][N] with the rows of the solved wires filled in,
        w = (<a,(1,x)> * <b,(1,x)> - <c,(1,x)> without w) * k^-1   per limb and slot, canonical.
    Reads given and already solved rows only; rows of unsolved wires are returned as they were."""
    out = np.array(assignment, dtype=np.uint64)
    assert out.ndim == 3 and out.shape[0] == cs.n_vars and out.shape[1] == len(q), out.shape
    for j, t in solve_schedule(cs, given, q)[0]:
        _solve_step(cs, out, j, t, q)
    return out


class HintReport(collections.namedtuple("HintReport", "n_bits_bad bad_hint bad_limb bad_slot n_zero zero_hint zero_limb zero_slot")):
    """What a hinted solve reports (rs_solve_hint_report of ringsnark_amd/solve_hints.h): bad positions (hint, limb, slot) of
    BITS hints and zero source positions of INV and QUOT hints, with the first of each: lowest hint, then lowest
    limb*N + slot; zeros when there is none.  Both are answers, not errors."""
    __slots__ = ()

    @property
    def clean(self):
        return self.n_bits_bad == 0 and self.n_zero == 0


def solve_hinted(cs: R1CS, given, hints, assignment, q: List[int]):
    """The solver with hints on the host in exact Python integers, the host mirror of rs_r1cs_solve_hinted: a copy of
    `assignment` [n_vars][L][N] with the rows of the solved wires filled in, constraint steps as solve does, hint steps by
    bit_decompose and inv_or_zero.  Returns (assignment, HintReport)."""
    hints = list(hints)
    out = np.array(assignment, dtype=np.uint64)
    assert out.ndim == 3 and out.shape[0] == cs.n_vars and out.shape[1] == len(q), out.shape
    n_bad = n_zero = 0
    first_bad = first_zero = None  # (hint, limb, slot)
    for kind, i, t in solve_hinted_schedule(cs, given, hints, q)[0]:
        if kind == 0:
            _solve_step(cs, out, i, t, q)
            continue
        h = hints[i]
        if h.kind == RS_HINT_BITS:
            bits, rep = bit_decompose(out[h.src], h.nbits, q)
            for k, v in enumerate(h.targets):
                out[v] = bits[k]
            n_bad += rep.n_bad
            if rep.n_bad:
                first_bad = min(first_bad or (i, rep.first_limb, rep.first_slot), (i, rep.first_limb, rep.first_slot))
        else:
            out[h.dst], rep = inv_or_zero(out[h.src], q, num=out[h.num] if h.kind == RS_HINT_QUOT else None)
            assert rep.clean, "a source row holds a word that is not a canonical residue"
            n_zero += rep.n_zero
            if rep.n_zero:
                first_zero = min(first_zero or (i, rep.zero_limb, rep.zero_slot), (i, rep.zero_limb, rep.zero_slot))
    return out, HintReport(n_bad, *(first_bad or (0, 0, 0)), n_zero, *(first_zero or (0, 0, 0)))


def running_max_r1cs(q: List[int], nbits: int, count: int):
    """The running maximum of x_0 .. x_count by comparisons on nbits-bit differences.  Public wires: `one` (variable 0,
    0-based), x_0 .. x_count (variables 1 .. count + 1).  Stage j < count has the wires s_j, b_{j,0} .. b_{j,nbits-1}, m_j
    (variables count + 2 + j (nbits + 2) ..), with m_{-1} = x_0, and the constraints
        (m_{j-1} - x_{j+1} + 2^(nbits-1) one) * one = s_j
        b_{j,k} * (one - b_{j,k}) = 0                      once per bit
        s_j * one = sum_k 2^k b_{j,k}
        b_{j,nbits-1} * (m_{j-1} - x_{j+1}) = m_j - x_{j+1}
    and the hint BITS(s_j -> b_j): 3 count levels, which alternate constraint, hint, constraint.  For inputs below
    2^(nbits-1), m_j = max(x_0 .. x_{j+1}).  Returns (R1CS, [Hint])."""
    assert nbits >= 2 and count >= 1
    rows = {"a": [], "b": [], "c": []}

    def add(a, b, c):
        rows["a"].append(a), rows["b"].append(b), rows["c"].append(c)

    one, hints, prev = 1, [], 2
    for j in range(count):
        x = 3 + j
        s = count + 3 + j * (nbits + 2)
        b = [s + 1 + k for k in range(nbits)]
        mx = s + 1 + nbits
        add([(prev, 1), (x, -1), (one, 1 << (nbits - 1))], [(one, 1)], [(s, 1)])
        for k in range(nbits):
            add([(b[k], 1)], [(one, 1), (b[k], -1)], [])
        add([(s, 1)], [(one, 1)], [(b[k], 1 << k) for k in range(nbits)])
        add([(b[-1], 1)], [(prev, 1), (x, -1)], [(mx, 1), (x, -1)])
        hints.append(Hint.bits(s - 1, b[0] - 1, nbits))
        prev = mx
    return from_rows(count * (nbits + 3), count + 2 + count * (nbits + 2), count + 2, rows, q), hints


def running_max_layout(nbits: int, count: int):
    """0-based variables of running_max_r1cs: (s_j, first bit of stage j, m_j) for every stage."""
    return [(count + 2 + j * (nbits + 2), count + 3 + j * (nbits + 2), count + 3 + j * (nbits + 2) + nbits) for j in range(count)]


def continued_fraction_r1cs(q: List[int], count: int):
    """y_{j+1} = c_j / (y_j + d_j), `count` times.  Public wires: `one` (variable 0, 0-based), y_0 (1), then c_j, d_j
    (2 + 2j, 3 + 2j).  Stage j has the wires t_j, y_{j+1} (variables 2 + 2 count + 2j ..) and the constraints
        (y_j + d_j) * one = t_j,      y_{j+1} * t_j = c_j
    and the hint QUOT(c_j, t_j -> y_{j+1}): 2 count levels, all slot-local.  Where t_j is zero y_{j+1} is 0, and the second
    constraint holds only if c_j is zero there too.  Returns (R1CS, [Hint])."""
    assert count >= 1
    rows = {"a": [], "b": [], "c": []}
    one, hints, y = 1, [], 2
    for j in range(count):
        c, d = 3 + 2 * j, 4 + 2 * j
        t = 3 + 2 * count + 2 * j
        rows["a"] += [[(y, 1), (d, 1)], [(t + 1, 1)]]
        rows["b"] += [[(one, 1)], [(t, 1)]]
        rows["c"] += [[(t, 1)], [(c, 1)]]
        hints.append(Hint.quot(c - 1, t - 1, t))
        y = t + 1
    return from_rows(2 * count, 2 + 4 * count, 2 + 2 * count, rows, q), hints


def chain_r1cs(m: int, q: List[int]) -> R1CS:
    """x_i * x_{i+1} = x_{i+2}, i < m; variables x_0..x_{m+1}; x_0, x_1 public (n_aux = m)."""
    rows = {"a": [[(i + 1, 1)] for i in range(m)], "b": [[(i + 2, 1)] for i in range(m)], "c": [[(i + 3, 1)] for i in range(m)]}
    return from_rows(m, m + 2, 2, rows, q)


def wide_r1cs(m: int, q: List[int], seed: int = 11, width: int = 8, n_inputs: int = 2) -> R1CS:
    """(sum of `width` earlier variables with small signed coefficients, plus a constant)
    * (x_{i+1}) = x_{i+2}.  Exercises multi-term linear combinations, the constant-one column
    and negative coefficients."""
    rng = np.random.RandomState(seed)
    rows = {"a": [], "b": [], "c": []}
    for i in range(m):
        terms = [(0, int(rng.randint(1, 5)))]
        for _ in range(width):
            terms.append((int(rng.randint(1, i + 3)), int(rng.randint(-3, 4)) or 1))
        rows["a"].append(terms)
        rows["b"].append([(i + 2, 1)])
        rows["c"].append([(i + 3, 1)])
    return from_rows(m, m + 2, n_inputs, rows, q)


def wide_poly_r1cs(m: int, q: List[int], N: int, seed: int = 17, width: int = 4, n_inputs: int = 2, aux_only: bool = False,
                   constants: bool = True) -> R1CS:
    """wide_r1cs with general ring elements among the coefficients: in `a` one polynomial coefficient per row on an
    arbitrary earlier variable (primary inputs included) and, on every third row, on the constant one; in `b` a
    polynomial coefficient on x_{i+1} on every other row:  <a_i, x> * (u_i x_{i+1}) = x_{i+2}.  Exercises every place
    a coefficient is read (evaluate in its three modes, the constant part of the mid vectors, the instance map).
    aux_only: polynomial coefficients multiply auxiliary variables only (the constant one and the primary inputs keep
    slot-constant scalars, so the device keeps its linear-form io vectors).  constants = False: no term on the constant
    one (the reference's witness map counts such terms in BOTH its io and its mid pass, r1cs_to_qrp.tcc:175-201, so a
    circuit with constants does not pass the reference's own verifier; end-to-end tests use circuits without them)."""
    rng = np.random.RandomState(seed)
    rand_ring = lambda: np.stack([rng.randint(0, p, N, dtype=np.int64).astype(np.uint64) for p in q])
    rows = {"a": [], "b": [], "c": []}
    for i in range(m):
        terms = [(0, rand_ring() if i % 3 == 0 and not aux_only else int(rng.randint(1, 5)))] if constants else []
        for k in range(width):
            idx = int(rng.randint(1, i + 3))
            poly = k == 0 and not (aux_only and idx <= n_inputs)
            terms.append((idx, rand_ring() if poly else (int(rng.randint(-3, 4)) or 1)))
        rows["a"].append(terms)
        rows["b"].append([(i + 2, rand_ring() if i % 2 == 0 and not (aux_only and i + 2 <= n_inputs) else 1)])
        rows["c"].append([(i + 3, 1)])
    return from_rows(m, m + 2, n_inputs, rows, q)


def dft_r1cs(q: List[int], N: int, root_pows: np.ndarray) -> R1CS:
    """The ONE-constraint circuit of the reference's benchmarks/bench_ntt_SEAL.cpp:28-55 (BASELINE.json configs[0]):
    N + 1 variables, all of them primary inputs (:28-29,37);  (x_1 + sum_{i=1}^{N-1} row^i * x_{i+1}) * 1 = x_{N+1}
    with row^i the i-th slot-wise power of the ring element `rs` whose residues are root_pows (:40-53).  root_pows:
    uint64 [L][N] (the reference fills it with the powers of the first prime's minimal 2N-th root of unity)."""
    rs = np.ascontiguousarray(root_pows, dtype=np.uint64)
    assert rs.shape == (len(q), N)
    qa = [int(p) for p in q]
    terms = [(1, 1)]
    row = rs.copy()
    for i in range(1, N):
        terms.append((i + 1, row.copy()))
        row = np.stack([(row[l].astype(object) * rs[l].astype(object) % qa[l]).astype(np.uint64) for l in range(len(q))])
    rows = {"a": [terms], "b": [[(0, 1)]], "c": [[(N + 1, 1)]]}
    return from_rows(1, N + 1, N + 1, rows, q)


def solve_forward(cs: R1CS, x0, x1, ring_mul, ring_lincomb):
    """Fill the assignment of chain/wide circuits: x_{i+2} = <a_i, x> * <b_i, x>  (b_i = x_{i+1}, possibly scaled).

    ring_lincomb(terms, assignment_list) and ring_mul(a, b) are supplied by the caller (CPU
    oracle in tests, device ring ops in the bench)."""
    asg = [x0, x1]
    rp, col, _ = cs.mats["a"]
    for i in range(cs.m):
        asg.append(ring_mul(ring_lincomb("a", i, asg), ring_lincomb("b", i, asg)))
    return asg


def logreg_r1cs(q: List[int], num_features: int = 256) -> R1CS:
    """The circuit of the reference's benchmarks/bench_logistic_regression_inference.cpp:72-125 (BASELINE.json
    configs[4]), variable for variable: per feature i two input ciphertexts in1[i], in2[i] of two ring elements each
    (allocated interleaved, :78-82), five outputs, the four products per feature, s02 and s11.  With 256 features:
    1031 constraints, 2055 variables, set_input_sizes(2*256+5 = 517) (:72,85).

      per feature (:94-107)   in1[i][0]*in2[i][0] = p00[i];  in1[i][0]*in2[i][1] = p01[i];
                              in1[i][1]*in2[i][0] = p10[i];  in1[i][1]*in2[i][1] = p11[i]
      sums (linear)           s0 = sum p00,  s1 = sum (p01 + p10),  s2 = sum p11     (the ciphertext product's components)
      degree-2 sigmoid (:116-125)  s0*s0 = out0;  (2 s0)*s1 = out1;  s0*s2 = s02;  s1*s1 = s11;
                              1 * (2 s02 + s11) = out2;  s1*s2 = out3;  s2*s2 = out4
    Variable k (1-based, 0 = the constant one): in1[i][j] = 4i+1+j, in2[i][j] = 4i+3+j, out[k] = 4F+1+k,
    p00[i] = 4F+6+i, p01[i] = 5F+6+i, p10[i] = 6F+6+i, p11[i] = 7F+6+i, s02 = 8F+6, s11 = 8F+7."""
    F = num_features
    in1 = lambda i, j: 4 * i + 1 + j
    in2 = lambda i, j: 4 * i + 3 + j
    out = lambda k: 4 * F + 1 + k
    p = lambda which, i: (4 + which) * F + 6 + i
    s02, s11 = 8 * F + 6, 8 * F + 7
    rows = {"a": [], "b": [], "c": []}

    def add(a, b, c):
        rows["a"].append(a)
        rows["b"].append(b)
        rows["c"].append(c)

    for i in range(F):
        add([(in1(i, 0), 1)], [(in2(i, 0), 1)], [(p(0, i), 1)])
        add([(in1(i, 0), 1)], [(in2(i, 1), 1)], [(p(1, i), 1)])
        add([(in1(i, 1), 1)], [(in2(i, 0), 1)], [(p(2, i), 1)])
        add([(in1(i, 1), 1)], [(in2(i, 1), 1)], [(p(3, i), 1)])
    s0 = [(p(0, i), 1) for i in range(F)]
    s1 = sorted([(p(1, i), 1) for i in range(F)] + [(p(2, i), 1) for i in range(F)])
    s2 = [(p(3, i), 1) for i in range(F)]
    add(s0, s0, [(out(0), 1)])
    add([(k, 2) for k, _ in s0], s1, [(out(1), 1)])
    add(s0, s2, [(s02, 1)])
    add(s1, s1, [(s11, 1)])
    add([(0, 1)], [(s02, 2), (s11, 1)], [(out(2), 1)])
    add(s1, s2, [(out(3), 1)])
    add(s2, s2, [(out(4), 1)])
    n_vars = 8 * F + 7
    return from_rows(4 * F + 7, n_vars, 2 * F + 5, rows, q)


def logreg_assignment(num_features, inputs, ring_mul, ring_add, ring_mul_scalar):
    """Full assignment [n_vars] of logreg_r1cs from the 4F input ring elements (in1[i][0], in1[i][1], in2[i][0],
    in2[i][1] per feature; bench_logistic_regression_inference.cpp:147-205).  The ring operations are supplied by
    the caller (CPU oracle in tests, batched device ops in the bench); they must accept leading batch dimensions."""
    F = num_features
    x = inputs.reshape((F, 4) + tuple(inputs.shape[1:]))
    a0, a1, b0, b1 = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    p00, p01, p10, p11 = ring_mul(a0, b0), ring_mul(a0, b1), ring_mul(a1, b0), ring_mul(a1, b1)

    def total(v):  # pairwise tree sum of F ring elements
        while v.shape[0] > 1:
            h = v.shape[0] // 2
            head = ring_add(v[:h], v[h:2 * h])
            v = head if v.shape[0] == 2 * h else _cat([head, v[2 * h:]])
        return v[0]

    s0, s1, s2 = total(p00), total(ring_add(p01, p10)), total(p11)
    s_02, s_11 = ring_mul(s0, s2), ring_mul(s1, s1)
    outs = [ring_mul(s0, s0), ring_mul(ring_mul_scalar(s0, 2), s1), ring_add(ring_mul_scalar(s_02, 2), s_11), ring_mul(s1, s2),
            ring_mul(s2, s2)]
    parts = [inputs] + [o[None] for o in outs] + [p00, p01, p10, p11, s_02[None], s_11[None]]
    return _cat(parts)


@dataclass
class BitsReport:
    """What a bit decomposition reports (rs_bits_report of ringsnark_amd/bits.h, field for field)."""
    n_bad: int  # bad ring-layout positions (element, limb, slot)
    first_elem: int  # lowest element with a bad position, then the lowest limb*N + slot in it; all 0 when there is none
    first_limb: int
    first_slot: int
    word: int  # the word at that position
    value: int  # the limb-0 word of that slot

    @property
    def clean(self):
        return self.n_bad == 0


def max_nbits(q: List[int]) -> int:
    """min_i floor(log2 q_i): every value below 2^max_nbits is a canonical residue in every limb."""
    return min(int(p).bit_length() - 1 for p in q)


def bit_decompose(x, nbits: int, q: List[int]):
    """The host mirror of rs_ring_bit_decompose (ringsnark_amd/bits.h), exact.  x: uint64 [count][L][N] (or one element
    [L][N]).  Per (element, slot), with v the limb-0 word: bits[e, k, :, slot] = (v >> k) & 1 in every limb, k < nbits.
    A position (element, limb i, slot) is bad when i == 0 and v >= 2^nbits, or i > 0 and the limb-i word differs from v.
    Returns (bits uint64 [count][nbits][L][N] (or [nbits][L][N]), BitsReport)."""
    x = np.asarray(x, dtype=np.uint64)
    single = x.ndim == 2
    xs = x[None] if single else x
    assert xs.ndim == 3 and xs.shape[1] == len(q), xs.shape
    assert 1 <= nbits <= max_nbits(q), "nbits must be between 1 and min_i floor(log2 q_i) = %d" % max_nbits(q)
    count, L, N = xs.shape
    v = xs[:, 0]
    ks = np.arange(nbits, dtype=np.uint64).reshape(1, nbits, 1, 1)
    bits = np.broadcast_to((v[:, None, None, :] >> ks) & np.uint64(1), (count, nbits, L, N)).copy()
    bad = xs != v[:, None, :]
    bad[:, 0] = (v >> np.uint64(nbits)) != 0
    n_bad = int(bad.sum())
    if n_bad == 0:
        rep = BitsReport(0, 0, 0, 0, 0, 0)
    else:
        key = int(np.argmax(bad.reshape(-1)))
        e, idx = divmod(key, L * N)
        limb, slot = divmod(idx, N)
        rep = BitsReport(n_bad, e, limb, slot, int(xs[e, limb, slot]), int(xs[e, 0, slot]))
    return (bits[0] if single else bits), rep


def plaintext_check_r1cs(q: List[int], logT: int, count: int = 1, constants: bool = False, n_inputs: Optional[int] = None) -> R1CS:
    """The range check by bit decomposition of the reference's examples/example_plaintext_check_SEAL.cpp:36-54 and
    benchmarks/bench_plaintext_check_SEAL.cpp:49-68, `count` times: count * (logT + 1) constraints.

    constants=False (the default): variable 1 is a public wire `one` (n_inputs = 1; the verifier supplies one = 1), and
    block p follows as b_{p,0} .. b_{p,logT-1}, x_p (variables 2 + p (logT+1) + i, 1-based):
        b_{p,i} * (one - b_{p,i}) = 0   for i < logT,      x_p * one = sum_i 2^i b_{p,i}.
    constants=True: the reference's file verbatim -- the constant one stands where `one` stood and no extra variable
    exists (block p: variables 1 + p (logT+1) + i): vars[i] * (1 - vars[i]) = 0, vars[logT] * 1 = sum (1 << i) vars[i].
    n_inputs defaults to 1 (the example, example_plaintext_check_SEAL.cpp:44); n_inputs = logT is the benchmark
    (bench_plaintext_check_SEAL.cpp:58).  Coefficients are the true 2^i mod q_l.  The benchmark's `(1 << i)`
    (bench_plaintext_check_SEAL.cpp:65, logT = 32) is evaluated in `int` and is NOT 2^31 at i = 31 (a negative value
    where the shift is defined at all); this generator does not reproduce that.
    The reference's own verifier REJECTS the constants=True form: its witness map counts terms on the constant one in
    both its io and its mid pass (r1cs_to_qrp.tcc:175-201), so with a satisfied assignment rinocchio::verifier fails
    exactly `L_beta = L` and `P = H Z(s)` (rinocchio.tcc:283-293).  The same circuit on the public wire `one` is accepted,
    which is why it is the default and what the end-to-end tests use."""
    assert logT >= 1 and count >= 1
    w = logT + 1
    rows = {"a": [], "b": [], "c": []}
    one = 0 if constants else 1
    first = 1 if constants else 2
    for p in range(count):
        b = [first + p * w + i for i in range(logT)]
        x = first + p * w + logT
        for i in range(logT):
            rows["a"].append([(b[i], 1)])
            rows["b"].append([(one, 1), (b[i], -1)])
            rows["c"].append([])
        rows["a"].append([(x, 1)])
        rows["b"].append([(one, 1)])
        rows["c"].append([(b[i], 1 << i) for i in range(logT)])
    n_vars = count * w + (0 if constants else 1)
    return from_rows(count * w, n_vars, 1 if n_inputs is None else n_inputs, rows, q)


def plaintext_check_layout(cs_or_logT, count: int, constants: bool = False):
    """(logT, first_bit_row): block p of a plaintext_check_r1cs assignment is rows first_bit_row + p (logT+1) ..,
    b_0 .. b_{logT-1} then x.  From the circuit itself (count blocks) or from logT and `constants`."""
    if isinstance(cs_or_logT, R1CS):
        cs = cs_or_logT
        assert cs.m % count == 0 and cs.n_vars - cs.m in (0, 1), "not a plaintext_check_r1cs of %d blocks" % count
        return cs.m // count - 1, cs.n_vars - cs.m
    return int(cs_or_logT), 0 if constants else 1


def plaintext_check_assignment(cs_or_logT, xs, q: List[int], constants: bool = False) -> np.ndarray:
    """The host assignment [n_vars][L][N] of plaintext_check_r1cs from the values xs [count][L][N] (every slot one
    integer below 2^logT, the same word in every limb): `one` (unless constants), then per block the bit rows and x."""
    xs = np.asarray(xs, dtype=np.uint64)
    assert xs.ndim == 3 and xs.shape[1] == len(q), xs.shape
    count = xs.shape[0]
    logT, first = plaintext_check_layout(cs_or_logT, count, constants)
    bits, _ = bit_decompose(xs, logT, q)
    asg = np.empty((first + count * (logT + 1),) + xs.shape[1:], dtype=np.uint64)
    asg[:first] = 1
    blocks = asg[first:].reshape((count, logT + 1) + xs.shape[1:])
    blocks[:, :logT] = bits
    blocks[:, logT] = xs
    return asg


class InvReport(collections.namedtuple("InvReport", "n_zero zero_elem zero_limb zero_slot n_bad bad_elem bad_limb bad_slot bad_x bad_num")):
    """What an inverse-or-zero reports (rs_inv_report of ringsnark_amd/inverse.h, field for field).  Zeros are ordinary
    input; clean: no word that is not a canonical residue."""
    __slots__ = ()

    @property
    def clean(self):
        return self.n_bad == 0


def inv_or_zero(x, q: List[int], num=None):
    """The host mirror of rs_ring_inv_or_zero (ringsnark_amd/inverse.h), exact (Python integers).  x: uint64 [count][L][N]
    (or one element [L][N]); num: None or the same shape.  Per position (element, limb i, slot): 0 < x < q_i gives
    x^-1 mod q_i, times num when given; x == 0 gives 0 and counts in n_zero; x >= q_i, or num >= q_i, gives 0 and counts
    in n_bad and not in n_zero.  The firsts are the lowest element, then the lowest limb*N + slot.
    Returns (out of x's shape, InvReport)."""
    x = np.asarray(x, dtype=np.uint64)
    single = x.ndim == 2
    xs = x[None] if single else x
    assert xs.ndim == 3 and xs.shape[1] == len(q), xs.shape
    ns = None
    if num is not None:
        ns = np.asarray(num, dtype=np.uint64)
        ns = ns[None] if single else ns
        assert ns.shape == xs.shape, (ns.shape, xs.shape)
    count, L, N = xs.shape
    out = np.zeros_like(xs)
    qs = np.array([int(p) for p in q], dtype=np.uint64).reshape(1, L, 1)
    bad = xs >= qs
    if ns is not None:
        bad |= ns >= qs
    zero = ~bad & (xs == 0)
    for e, l, s in zip(*np.nonzero(~bad & ~zero)):
        p = int(q[l])
        v = pow(int(xs[e, l, s]), p - 2, p)
        out[e, l, s] = v if ns is None else v * int(ns[e, l, s]) % p
    fields = [int(zero.sum()), 0, 0, 0, int(bad.sum()), 0, 0, 0, 0, 0]
    if fields[0]:
        e, idx = divmod(int(np.argmax(zero.reshape(-1))), L * N)
        fields[1:4] = [e, idx // N, idx % N]
    if fields[4]:
        e, idx = divmod(int(np.argmax(bad.reshape(-1))), L * N)
        limb, slot = divmod(idx, N)
        fields[5:10] = [e, limb, slot, int(xs[e, limb, slot]), 0 if ns is None else int(ns[e, limb, slot])]
    return (out[0] if single else out), InvReport(*fields)


def is_zero_r1cs(q: List[int], count: int = 1) -> R1CS:
    """The is-zero gadget, `count` times.  Variable 1 is the public wire `one` (n_inputs = 1; plaintext_check_r1cs says why
    a public wire and not the constant); block p is x_p, inv_p, z_p (variables 2 + 3p .. 4 + 3p, 1-based):
        constraint 2p:      x_p * inv_p = one - z_p
        constraint 2p + 1:  x_p * z_p   = 0
    so z_p is 1 in the slots where x_p is zero and 0 elsewhere, and inv_p is the inverse-or-zero of x_p.  With one, x_p
    and inv_p given the solver finds z_p through the c side of constraint 2p."""
    assert count >= 1
    rows = {"a": [], "b": [], "c": []}
    for p in range(count):
        x, inv, z = 2 + 3 * p, 3 + 3 * p, 4 + 3 * p
        rows["a"] += [[(x, 1)], [(x, 1)]]
        rows["b"] += [[(inv, 1)], [(z, 1)]]
        rows["c"] += [[(1, 1), (z, -1)], []]
    return from_rows(2 * count, 1 + 3 * count, 1, rows, q)


def is_zero_assignment(xs, q: List[int]) -> np.ndarray:
    """The host assignment [1 + 3 count][L][N] of is_zero_r1cs from the values xs [count][L][N] (canonical residues): `one`,
    then per block x, its inverse-or-zero and the zero indicator."""
    xs = np.asarray(xs, dtype=np.uint64)
    assert xs.ndim == 3 and xs.shape[1] == len(q), xs.shape
    inv, rep = inv_or_zero(xs, q)
    assert rep.clean, "x holds a word that is not a canonical residue"
    asg = np.empty((1 + 3 * xs.shape[0],) + xs.shape[1:], dtype=np.uint64)
    asg[0] = 1
    blocks = asg[1:].reshape((xs.shape[0], 3) + xs.shape[1:])
    blocks[:, 0] = xs
    blocks[:, 1] = inv
    blocks[:, 2] = xs == 0
    return asg


def division_r1cs(q: List[int], count: int = 1) -> R1CS:
    """Slotwise division, `count` times.  Variable 1 is the public wire `one`; block p is a_p, b_p, binv_p, y_p (variables
    2 + 4p .. 5 + 4p, 1-based):
        constraint 2p:      b_p * binv_p = one     (b_p is invertible in every slot)
        constraint 2p + 1:  y_p * b_p    = a_p"""
    assert count >= 1
    rows = {"a": [], "b": [], "c": []}
    for p in range(count):
        a, b, binv, y = 2 + 4 * p, 3 + 4 * p, 4 + 4 * p, 5 + 4 * p
        rows["a"] += [[(b, 1)], [(y, 1)]]
        rows["b"] += [[(binv, 1)], [(b, 1)]]
        rows["c"] += [[(1, 1)], [(a, 1)]]
    return from_rows(2 * count, 1 + 4 * count, 1, rows, q)


def division_assignment(a, b, q: List[int]) -> np.ndarray:
    """The host assignment [1 + 4 count][L][N] of division_r1cs from a, b [count][L][N] (canonical residues): `one`, then
    per block a, b, the inverse-or-zero of b and the quotient a / b (0 where b is zero: such a slot violates constraint
    2p)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    assert a.shape == b.shape and b.ndim == 3 and b.shape[1] == len(q), (a.shape, b.shape)
    binv, rep = inv_or_zero(b, q)
    y, rep_y = inv_or_zero(b, q, num=a)
    assert rep.clean and rep_y.clean, "a or b holds a word that is not a canonical residue"
    asg = np.empty((1 + 4 * b.shape[0],) + b.shape[1:], dtype=np.uint64)
    asg[0] = 1
    blocks = asg[1:].reshape((b.shape[0], 4) + b.shape[1:])
    blocks[:, 0] = a
    blocks[:, 1] = b
    blocks[:, 2] = binv
    blocks[:, 3] = y
    return asg


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.ascontiguousarray(np.concatenate(parts))
    import torch
    return torch.cat(parts).contiguous()
