"""Shared builders for the parity tests (CPU oracle side)."""
from fractions import Fraction

import numpy as np

from oracle import oracle as O
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R


def oracle_ctx(prm):
    return O.Ctx(prm.N, prm.q, prm.N_enc, prm.Q)


def oracle_cs(cs):
    return O.R1CSHandle(cs.m, cs.n_vars, cs.n_inputs, cs.mats, cs.poly_idx, cs.poly_table)


def lincomb_oracle(ctx, cs):
    def f(name, i, asg):
        rp, col, cf = cs.mats[name]
        acc = np.zeros(ctx.ring_shape(), dtype=np.uint64)
        pidx = cs.poly_idx[name] if cs.poly_idx is not None else None
        for e in range(rp[i], rp[i + 1]):
            if pidx is not None and pidx[e] >= 0:
                coeff = cs.poly_table[pidx[e]]
            else:
                coeff = np.stack([np.full(ctx.N, cf[l, e], dtype=np.uint64) for l in range(ctx.L)])
            v = ctx.ring_scalar(1) if col[e] == 0 else asg[col[e] - 1]
            acc = ctx.ring_add(acc, ctx.ring_mul(v, coeff))
        return acc
    return f


def make_assignment(ctx, cs, seed=7):
    x0, x1 = ctx.random_ring(seed), ctx.random_ring(seed + 1)
    asg = R.solve_forward(cs, x0, x1, ctx.ring_mul, lincomb_oracle(ctx, cs))
    return np.ascontiguousarray(np.stack(asg))


def limb_slices(ctx, vec):
    """[t][L][N] -> list over limbs of contiguous [t][N]."""
    return [np.ascontiguousarray(vec[:, i, :]) for i in range(ctx.L)]


def dft_circuit(prm, ctx, seed=5):
    """The statement of the reference's benchmarks/bench_ntt_SEAL.cpp:28-83 on the ring of `prm`: the one-constraint
    DFT circuit (ringsnark_amd.r1cs.dft_r1cs) with root_pows = powers of the minimal primitive 2N-th root of unity of
    the FIRST ring prime (:40-47; for the other limbs the same integers are reduced mod q_i -- the reference hands a
    vector of N words to a constructor that adopts L*N, so what it holds there is not defined), and a satisfying
    assignment: x_1..x_N Scalars (the reference's plaintext coefficients, :70-75), x_{N+1} = the evaluated sum (:77-78).
    Returns (cs, assignment [N+1][L][N])."""
    N, q0 = prm.N, int(prm.q[0])
    root = O.minimal_primitive_root(2 * N, q0)
    pw = [1]
    for _ in range(N - 1):
        pw.append(pw[-1] * root % q0)
    root_pows = np.array([[v % int(p) for v in pw] for p in prm.q], dtype=np.uint64)
    cs = R.dft_r1cs(prm.q, N, root_pows)
    rng = np.random.RandomState(seed)
    xs = [ctx.ring_scalar(int(v)) for v in rng.randint(0, 2**16, N)]
    xs.append(lincomb_oracle(ctx, cs)("a", 0, xs))
    return cs, np.ascontiguousarray(np.stack(xs))


# ---- sign-aligned worst-case inputs for the inner-product kernels (tests/test_aligned_inputs.py, tests/test_msm_worst_case.py)
_NTT = {}


def _ntt(logn, Q):
    if (logn, Q) not in _NTT:
        _NTT[(logn, Q)] = O.NTT(logn, Q)
    return _NTT[(logn, Q)]


def centred_lift(plain, q):
    """Canonical residues mod q (uint64) -> their balanced representatives (int64): c >= (q + 1) / 2 => c - q."""
    lift = np.asarray(plain, dtype=np.uint64).astype(np.int64)
    lift[lift >= (q + 1) // 2] -= q
    return lift


def plain_spectrum(ctx, j, lift):
    """NTT_{Q_j}(lift mod Q_j) of a row of signed integers [N_enc]: the factor u the kernels multiply a key word by."""
    Q = ctx.Q[j]
    return _ntt(ctx.N_enc.bit_length() - 1, Q).fwd((np.asarray(lift, dtype=np.int64) % np.int64(Q)).astype(np.uint64))


def term_spectra(ctx, rings, kinds=None, slot_const=False):
    """u [D][L][K][N_enc] (uint64) of the terms of one coefficient vector.  rings: [D][L][N]; slot_const: [D][L] values (the
    ring element holds the value in each of its N slots: with N == N_enc its plaintext is the constant polynomial);
    kinds[d] == KIND_ONE: the plaintext is the constant polynomial 1, the spectrum all ones."""
    D = len(rings)
    U = np.empty((D, ctx.L, ctx.K, ctx.N_enc), dtype=np.uint64)
    for d in range(D):
        for i in range(ctx.L):
            if kinds is not None and kinds[d] == O.KIND_ONE:
                lift = None
            elif slot_const:  # N == N_enc: the constant polynomial, whose spectrum is the lifted constant everywhere
                lift = centred_lift(ctx.batch_encode(i, np.full(ctx.N, rings[d][i], dtype=np.uint64)), ctx.q[i])
            else:
                lift = centred_lift(ctx.batch_encode(i, rings[d][i]), ctx.q[i])
            for j in range(ctx.K):
                if lift is None:
                    U[d, i, j] = 1
                else:
                    U[d, i, j] = plain_spectrum(ctx, j, lift)
    return U


def aligned_sign(i, c, j):
    """Sign of every target of slab (limb i, component c, prime j): both signs occur in every call (c takes both values)."""
    return 1 if (i + c + j) % 2 == 0 else -1


def aligned_key(ctx, U, seed, frac=0.30):
    """Key words that turn the spectra U [D][L][K][N_enc] (no zero entry) into chosen products: returns (encs
    [D][L][2][K][N_enc] uint64, targets, Python integers in the same shape) with
        target = s (floor(frac Q_j) - r[pos]),  r uniform in [0, 2^20),  s = aligned_sign(i, c, j),
        ct     = target u^-1 mod Q_j,
    so that ct u = target (mod Q_j) at every position and all targets of a slab carry one sign."""
    D = U.shape[0]
    rng = np.random.RandomState(seed)
    encs = np.empty(ctx.enc_shape(D), dtype=np.uint64)
    targets = np.empty(ctx.enc_shape(D), dtype=object)
    for j, Q in enumerate(ctx.Q):
        base = int(Fraction(frac) * Q)  # floor(frac Q_j), exactly
        for d in range(D):
            for i in range(ctx.L):
                uinv = np.array([pow(int(x), -1, Q) for x in U[d, i, j]], dtype=object)
                for c in range(2):
                    r = rng.randint(0, 1 << 20, size=ctx.N_enc).astype(np.int64)
                    tgt = (aligned_sign(i, c, j) * (base - r)).astype(object)
                    targets[d, i, c, j] = tgt
                    encs[d, i, c, j] = (tgt * uinv % Q).astype(np.uint64)
    return encs, targets


def aligned_terms(ctx, D, seed, frac=0.30, kinds=None, slot_const=False, rings=None):
    """D terms of an inner product whose every product is a chosen balanced integer of one sign per slab, so that the
    sum over T terms is as large as T terms can make it.  Returns (rings [D][L][N], encs [D][L][2][K][N_enc], targets); see
    aligned_key for encs and targets.  The plaintext rows are free (random ring elements from `seed`, redrawn while a
    spectrum has a zero; or `rings`, an array or -- the vectors of one group, whose lifts the kernels add -- a list of
    arrays); u = NTT_{Q_j}(centred_lift(batch_encode(i, rings[d, i])) mod Q_j) comes from the CPU oracle.  kinds and
    slot_const as in term_spectra (slot_const: rings is [D][L]).

    Why frac = 0.30: f64mod.hpp bounds the quotient error of mulmod(a, b) by 3 * 2^-53 * |a b / p|.  Here a is a canonical
    key word (< p) and b the kernel's representative of u with |b| <= 2^49, so |a b / p| <= 2^49 and the error is at most
    3 * 2^-4 = 0.1875.  a b / p = integer + target / p with |target / p| <= 0.30, and 0.30 + 0.1875 < 0.5: the rounded
    quotient is that integer and the kernel's product is exactly `target`, whichever lazy representative of u it holds.
    The expected sum therefore needs no oracle (closed_form), and an accumulator that is never reduced holds exactly the
    running sum of the targets.  Primes in [2^49, 2^50) (the *q50 contexts, toy50): with a centred b (|b| <= p / 2) the same
    holds; with a lazier representative, |b| up to p, the error bound is 0.375 and a product may come out as target -+ p
    (f64mod.hpp's second regime, |r| <= 0.875 p).  It is the same residue, so closed_form is still the expected value, and
    what makes the sums large is the condition check_aligned_inputs asserts on the targets."""
    if rings is None:
        if slot_const:
            rng = np.random.RandomState(seed + 1)
            rings = np.stack([rng.randint(1, 2**62, size=D, dtype=np.int64).astype(np.uint64) % np.uint64(q) for q in ctx.q], axis=1)
            rings[rings == 0] = 1
        else:
            rings = ctx.random_ring(seed + 1, D)
            if kinds is not None:
                for d in range(D):
                    if kinds[d] == O.KIND_ONE:
                        rings[d] = ctx.ring_scalar(1)
        U, redraw = term_spectra(ctx, rings, kinds, slot_const), 0
        while not U.all():
            for d in sorted(set(np.argwhere(U == 0)[:, 0])):
                redraw += 1
                rings[d] = rings[d] + np.uint64(1) if slot_const else ctx.random_ring(seed + 1 + 7919 * redraw)
                U[d] = term_spectra(ctx, rings[d:d + 1], slot_const=slot_const)[0]
    else:
        group = rings if isinstance(rings, (list, tuple)) else [rings]
        U = np.zeros((D, ctx.L, ctx.K, ctx.N_enc), dtype=np.uint64)
        for vec in group:
            Uv = term_spectra(ctx, vec, kinds, slot_const)
            for j, Q in enumerate(ctx.Q):
                U[:, :, j] = (U[:, :, j] + Uv[:, :, j]) % np.uint64(Q)  # the transform is linear; both summands < 2^60
        assert U.all(), "a spectrum of the given rows has a zero: no key word can produce the target there"
    encs, targets = aligned_key(ctx, U, seed, frac)
    return rings, encs, targets


def aligned_T(Q, frac=0.30, margin=4):
    """Number of same-sign terms after which an accumulator that is never reduced has left the exactly representable
    integers: ceil(2^53 / (frac min(Q) - 2^20)) + margin."""
    assert margin >= 4
    per_term = Fraction(frac) * min(int(x) for x in Q) - (1 << 20)
    return -((-(1 << 53) * per_term.denominator) // per_term.numerator) + margin


def closed_form(ctx, targets, T):
    """sum_t targets[t % D] mod Q_j in Python integers: the inner product of T aligned terms, [L][2][K][N_enc] uint64."""
    D = targets.shape[0]
    counts = np.bincount(np.arange(T) % D, minlength=D)
    out = np.empty(ctx.enc_shape(), dtype=np.uint64)
    for j, Q in enumerate(ctx.Q):
        s = sum(int(counts[d]) * targets[d, :, :, j] for d in range(D))
        out[:, :, j] = (s % Q).astype(np.uint64)
    return out


def check_aligned_inputs(ctx, targets, T, frac=0.30):
    """The conditions on aligned inputs that give a kernel test its meaning, per (limb, component, prime) slab: every
    |target| <= frac Q_j, one sign, and the running sum over T cyclic terms -- what an accumulator without periodic
    reduction would hold -- beyond 2^53 in absolute value at some position.  Returns the smallest of the slabs' largest
    |running sum| / 2^53."""
    D, reached = targets.shape[0], []
    for i in range(ctx.L):
        for c in range(2):
            for j, Q in enumerate(ctx.Q):
                slab = np.stack([targets[d, i, c, j].astype(np.int64) for d in range(D)])
                assert all(abs(int(v)) <= Fraction(frac) * Q for v in (slab.min(), slab.max())), (i, c, j)
                assert (np.sign(slab) == aligned_sign(i, c, j)).all(), (i, c, j)
                assert T * int(np.abs(slab).max()) < 2**62  # the int64 running sum below is exact
                run, peak = np.zeros(slab.shape[1], dtype=np.int64), 0
                for t in range(T):
                    run += slab[t % D]
                    peak = max(peak, int(np.abs(run).max()))
                assert peak > 2**53, (i, c, j, peak / 2.0**53)
                reached.append(peak / 2.0**53)
    return min(reached)


EXTREME_PATTERNS = ("plus", "minus", "alternating", "random")


def extreme_rows(ctx, limb, pattern, seed=0):
    """The ring-element row [N] (N == N_enc) whose plaintext has every coefficient at the ends of the balanced range:
    (q - 1) / 2 (lift +(q - 1) / 2) or (q + 1) / 2 (lift -(q - 1) / 2).  pattern: one of EXTREME_PATTERNS."""
    assert ctx.N == ctx.N_enc, "every plaintext is a batch encoding only when N == N_enc"
    q, n = ctx.q[limb], ctx.N_enc
    if pattern == "plus":
        minus = np.zeros(n, dtype=bool)
    elif pattern == "minus":
        minus = np.ones(n, dtype=bool)
    elif pattern == "alternating":
        minus = np.arange(n) % 2 == 1
    else:
        assert pattern == "random", pattern
        minus = np.random.RandomState(seed).randint(0, 2, size=n).astype(bool)
    poly = np.where(minus, np.uint64((q + 1) // 2), np.uint64((q - 1) // 2)).astype(np.uint64)
    return ctx.batch_decode(limb, poly)


# The contexts of tests/test_msm_worst_case.py, smallest at which each kernel exists: name -> make_params arguments (None: preset)
WORST_CASES = {
    "toy49": None,
    "n2048": (2048, [43], 2048, [49, 48]),
    "n8192": (8192, [43], 8192, [49, 48]),
    "n16384": (2048, [43], 16384, [49, 48]),
    "n8192q44": (8192, [43], 8192, [44]),
    "hybrid8192": (8192, [54], 8192, [49, 48]),
    "n16384full": (16384, [43], 16384, [49, 48]),  # N == N_enc at 16384 points: extreme plaintext rows
    # the same kernel families on primes just below 2^50, the largest the FP64 arithmetic accepts: acc_period is 4 there
    "toy50": None,
    "n2048q50": (2048, [43], 2048, [50, 50]),
    "n8192q50": (8192, [50], 8192, [50, 50]),  # N == N_enc: extreme rows of a 50-bit ring prime, +-2 (q - 1) is about 2^51
    "n16384q50": (2048, [43], 16384, [50, 50]),
    "hybrid8192q50": (8192, [54], 8192, [50, 50]),
}
# the order the seeds of aligned_case / extreme_case count in: names are only ever appended, so a case keeps its inputs
_SEED_ORDER = ("hybrid8192", "n16384", "n16384full", "n2048", "n8192", "n8192q44", "toy49",
               "toy50", "n2048q50", "n8192q50", "n16384q50", "hybrid8192q50")
assert sorted(_SEED_ORDER) == sorted(WORST_CASES)
ALIGNED_D = 8


def worst_case_params(name):
    args = WORST_CASES[name]
    return P.preset(name) if args is None else P.make_params(*args, name=name)


_ALIGNED = {}


def aligned_case(name, variant="poly", key=0):
    """(ctx, rings, encs, targets, T, kinds) of a worst-case context, built once per process.  variant: "poly" (random ring
    elements), "one" (every term KIND_ONE), "const" (slot-constant vector: rings is [D][L]); key = 1: a second key, other
    targets, for the same rows."""
    if (name, variant, key) not in _ALIGNED:
        prm = worst_case_params(name)
        ctx = oracle_ctx(prm)
        T = aligned_T(prm.Q)
        seed = 1000 + 16 * _SEED_ORDER.index(name) + ("poly", "one", "const").index(variant)
        kinds = np.full(ALIGNED_D, O.KIND_ONE, dtype=np.uint8) if variant == "one" else None
        rings = aligned_case(name, variant)[1] if key else None
        rings, encs, targets = aligned_terms(ctx, ALIGNED_D, seed + 8 * key, kinds=kinds, slot_const=variant == "const", rings=rings)
        _ALIGNED[(name, variant, key)] = (ctx, rings, encs, targets, T, kinds)
    return _ALIGNED[(name, variant, key)]


EXTREME_CASES = {"n8192": 4, "hybrid8192": 1, "n16384full": 4, "n8192q50": 4}  # context -> vectors per group (MAX_GROUP_VECS; hybrid: one)


def extreme_case(name):
    """(ctx, rings [D][L][N], n_vecs, encs, targets, T): D terms whose rows come from extreme_rows, the four patterns in turn
    (the random one with a new seed each time), and the key aligned to the row a group of n_vecs copies of them sums to
    (every coefficient +-n_vecs (q - 1) / 2)."""
    if (name, "extreme") not in _ALIGNED:
        prm = worst_case_params(name)
        ctx = oracle_ctx(prm)
        n_vecs = EXTREME_CASES[name]
        rings = np.stack([np.stack([extreme_rows(ctx, i, EXTREME_PATTERNS[d % 4], seed=d) for i in range(ctx.L)]) for d in range(ALIGNED_D)])
        _, encs, targets = aligned_terms(ctx, ALIGNED_D, 2000 + _SEED_ORDER.index(name), rings=[rings] * n_vecs)
        _ALIGNED[(name, "extreme")] = (ctx, rings, n_vecs, encs, targets, aligned_T(prm.Q))
    return _ALIGNED[(name, "extreme")]


# ---- constructed noise polynomials for decode and the noise guard (tests/test_decode_boundaries.py) ---------------------
# A ciphertext (c0, c1) of the encoding scheme decrypts to the polynomial v = c0 + c1 s mod Q (Q = prod Q_j), centred into
# [-(Q - 1) / 2, (Q - 1) / 2]: its plaintext is v mod t, its noise budget max(0, bit_count(Q) - bit_count(max |v_x|) - 1).
# Here v is CHOSEN, so both are known in Python integers, and it is put where the device's exact comparisons (the sign, by
# the mixed-radix digits of floor(Q / 2); the bit length, by those of 2^b - 1) are ties or off a tie by one.
def enc_modulus(Qs):
    Q = 1
    for p in Qs:
        Q *= int(p)
    return Q


def noise_tb(Qs):
    """bit_count(Q): the number of threshold rows 2^b - 1, b < tb, of the device's guard"""
    return enc_modulus(Qs).bit_length()


def mixed_radix(Qs, value):
    """digits d_k of 0 <= value < Q with value = d_0 + Q_0 (d_1 + Q_1 (d_2 + ...))"""
    assert 0 <= value < enc_modulus(Qs)
    d = []
    for p in Qs:
        value, r = divmod(value, int(p))
        d.append(r)
    return d


def centred(w, Q):
    """the representative of w mod Q in [-(Q - 1) / 2, (Q - 1) / 2] (Q odd)"""
    w %= Q
    return w if w <= (Q - 1) // 2 else w - Q


def boundary_values(Qs, reduced=False):
    """[(kind, b, v)]: the centred integers v at which decoding and the guard decide by an exact comparison, no value twice.
    kind "half": the residues (Q - 3) / 2 .. (Q + 3) / 2 around floor(Q / 2), where the sign changes; "tie": |v| = 2^b - 1, 2^b
    or 2^b + 1, of either sign, around row b of the thresholds; "other": 0..3, -1, -2, and the residues 2^b + {-1, 0, 1} and
    Q - 2^b + {1, 0, -1} whose centred magnitude is not of that form (b = tb - 1).  b: every row 0 <= b < tb; reduced (the
    presets with many rows): the rows either side of the bit lengths of the partial products Q_0, Q_0 Q_1, .., where a
    threshold gains a digit, and 1, 2, tb - 3, tb - 2, tb - 1."""
    Q, tb = enc_modulus(Qs), noise_tb(Qs)
    if reduced:
        rows, part = {1, 2, tb - 3, tb - 2, tb - 1}, 1
        for p in Qs[:-1]:
            part *= int(p)
            rows |= {part.bit_length() - 1, part.bit_length(), part.bit_length() + 1}
        rows = sorted(rows)
    else:
        rows = range(tb)
    out, seen = [], set()

    def add(kind, b, w):
        if 0 <= w < Q and centred(w, Q) not in seen:
            seen.add(centred(w, Q))
            out.append((kind, b, centred(w, Q)))

    for w in ((Q - 3) // 2, (Q - 1) // 2, (Q + 1) // 2, (Q + 3) // 2):
        add("half", None, w)
    for b in rows:
        for w in ((1 << b) - 1, 1 << b, (1 << b) + 1, Q - (1 << b) + 1, Q - (1 << b), Q - (1 << b) - 1):
            add("tie" if 0 <= abs(centred(w, Q)) - ((1 << b) - 1) <= 2 and 0 <= w < Q else "other", b, w)
    for w in (0, 1, 2, 3, Q - 1, Q - 2):
        add("other", None, w)
    return out


def check_boundary_case(Qs, kind, b, v):
    """That a value of boundary_values is the case its kind says, in Python's mixed-radix digits.
    "tie": |v| >= 2^b is decided against the digits of 2^b - 1 -- by |v| > 2^b - 1 for v >= 0, by |v| - 1 >= 2^b - 1 for
    v < 0 (whose magnitude Q - w is one more than the digit-wise complement of the residue w): the compared number has the
    top K - 1 digits of 2^b - 1, and digit 0 alone holds the difference (-1, 0, 1 or 2).
    "half": the residue has the digits of floor(Q / 2), or differs from them by its distance in digit 0 alone."""
    Q = enc_modulus(Qs)
    assert abs(v) <= (Q - 1) // 2, (kind, b, v)
    if kind == "tie":
        c, thr = (v if v >= 0 else -v - 1), (1 << b) - 1
        assert -1 <= c - thr <= 2 and c >= 0, (b, v)
        dc, dt = mixed_radix(Qs, c), mixed_radix(Qs, thr)
        assert dc[1:] == dt[1:] and dc[0] - dt[0] == c - thr, (b, v, dc, dt)
    elif kind == "half":
        w, h = v % Q, (Q - 1) // 2
        dw, dh = mixed_radix(Qs, w), mixed_radix(Qs, h)
        assert abs(w - h) <= 2 and dw[1:] == dh[1:] and dw[0] - dh[0] == w - h, (v, dw, dh)
    else:
        assert kind == "other", kind


def poly_residues(ctx, v):
    """v mod Q_j of a polynomial of Python integers [N_enc]: uint64 [K][N_enc]"""
    v = np.asarray(v, dtype=object)
    assert v.shape == (ctx.N_enc,)
    return np.stack([(v % Q).astype(np.uint64) for Q in ctx.Q])


def noise_ciphertext(ctx, sk, v_per_limb, hidden, seed, plant=(), residues=None):
    """One encoding element [L][2][K][N_enc] whose limb i decrypts to exactly the polynomial v_per_limb[i] -- a Python integer
    (the constant polynomial) or N_enc of them -- with every |coefficient| <= (Q - 1) / 2:
        c1_j = a_j,   c0_j = NTT_{Q_j}(v mod Q_j) - a_j s_j  (mod Q_j).
    hidden False: a = 0 (the key plays no part); True: a uniform from `seed`, except at the positions `plant`, where a is
    solved for so that the words the device multiplies and adds are at the top of their range: c1 s = Q_j - 1 at the
    even-numbered ones, c0 = Q_j - 1 at the odd-numbered ones.  residues[i]: poly_residues of v_per_limb[i], if the
    caller has them."""
    n, Qfull = ctx.N_enc, enc_modulus(ctx.Q)
    out = np.zeros(ctx.enc_shape(), dtype=np.uint64)
    rng = np.random.RandomState(seed)
    for i, v in enumerate(v_per_limb):
        const = isinstance(v, int)
        assert (abs(v) if const else max(abs(x) for x in v)) <= (Qfull - 1) // 2
        res = None if const else (residues[i] if residues is not None else poly_residues(ctx, v))
        for j, Q in enumerate(ctx.Q):
            # the transform of a constant polynomial is that constant at every point
            u = np.full(n, v % Q, dtype=np.uint64) if const else _ntt(n.bit_length() - 1, Q).fwd(res[j])
            if not hidden:
                out[i, 0, j] = u
                continue
            a = rng.randint(0, Q, size=n, dtype=np.int64).astype(object)
            s = sk[j].astype(object)
            for k, x in enumerate(plant):
                assert s[x] != 0
                a[x] = ((Q - 1) if k % 2 == 0 else (int(u[x]) + 1)) * pow(int(s[x]), -1, Q) % Q
            out[i, 1, j] = a.astype(np.uint64)
            out[i, 0, j] = ((u.astype(object) - a * s) % Q).astype(np.uint64)
            for k, x in enumerate(plant):
                assert int(a[x]) * int(s[x]) % Q == Q - 1 if k % 2 == 0 else int(out[i, 0, j, x]) == Q - 1
    return out


def expected_budget(ctx, v_per_limb):
    """max(0, bit_count(Q) - bit_count(max_x |v_x|) - 1) per limb, in Python integers"""
    tb = noise_tb(ctx.Q)
    return [max(0, tb - (abs(v) if isinstance(v, int) else max(abs(x) for x in v)).bit_length() - 1) for v in v_per_limb]


def expected_decode(ctx, v_per_limb):
    """the ring element [L][N] an element of noise_ciphertext decodes to: limb i is the batch decoding of v mod q_i -- for a
    constant polynomial that constant in every slot, no oracle involved"""
    out = np.empty(ctx.ring_shape(), dtype=np.uint64)
    for i, v in enumerate(v_per_limb):
        if isinstance(v, int):
            out[i] = v % ctx.q[i]
        else:
            out[i] = ctx.batch_decode(i, (np.asarray(v, dtype=object) % ctx.q[i]).astype(np.uint64))
    return out
