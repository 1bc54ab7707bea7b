"""rs_enc_decode and rs_enc_noise_budget on CONSTRUCTED noise polynomials (builders and their host checks: tests/helpers.py).

Both rest on exact comparisons of Garner mixed-radix digits -- the sign of c0 + c1 s against the digits of floor(Q / 2), its bit
length against the digits of 2^b - 1 for the tb = bit_count(Q) rows b -- and random ciphertexts (the budget ladder of
tests/test_encoding.py) reach three or four of those rows and never a tie.  Here the noise polynomial v is chosen, the
ciphertext built around it (c1 = a, c0 = NTT(v) - a s), and the expectation is Python integers:
    budget = max(0, tb - bit_count(max |v_x|) - 1),   decode limb i = batch_decode(v mod q_i)  (a constant: v mod q_i).
Every value either side of every threshold row and of floor(Q / 2) occurs, in every limb, of either sign; the peak of a
general polynomial at the ends of a thread's stride; a spent element among good ones; a proof element with one bit of budget
through the two verifiers.  The CPU tests pin the builders against the oracle (whose budget composes multi-word integers and
whose decode centres by digits, like the device).  The last two tests are the encode side: the centred lift c >= (t + 1) / 2
=> c - t at its boundary.  All comparisons are integer equality."""
import functools
import os
import re

import numpy as np
import pytest

from ringsnark_amd import params as P
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["toy", "toy49", "toy50", "toy54", "toy60"]  # every threshold row; toy / toy49 / toy50: FP64, toy54 / toy60: the integer (Montgomery) arithmetic
BIG = ["C2", "C5"]                          # the reduced rows; C2: FP64, 8 coefficients per thread, C5: integer, 16
KERNEL = {"toy": "crt_decode_kernel", "toy49": "crt_decode_kernel", "toy50": "crt_decode_kernel", "C2": "crt_decode_kernel",
          "toy54": "crt_decode_kernel_int", "toy60": "crt_decode_kernel_int", "C5": "crt_decode_kernel_int"}
LIMB_STEP = 7  # limb i of element e of a sweep carries value e + 7 i of the list: no two limbs of an element hold the same value


# ---- shared inputs (CPU, built once) -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup(name):
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    return prm, ctx, ctx.keygen(9)


def enc_threads(logn):
    """threads of a decode workgroup, read from the library's source (csrc/rs_internal.hpp: enc_threads)"""
    src = open(os.path.join(ROOT, "ringsnark_amd", "csrc", "rs_internal.hpp")).read()
    m = re.search(r"inline int enc_threads\(int logn\) \{ return \(int\)std::max\((\d+), std::min\((\d+), \(1 << logn\) / (\d+)\)\); \}", src)
    assert m, "enc_threads has changed: restate it here"
    lo, hi, per = (int(x) for x in m.groups())
    return max(lo, min(hi, (1 << logn) // per))


def spread(vals, L):
    """elements [len(vals)][L] of constants: limb i of element e = vals[e + LIMB_STEP i]: every value in every limb"""
    n = len(vals)
    out = [[vals[(e + LIMB_STEP * i) % n] for i in range(L)] for e in range(n)]
    assert all(len(set(el)) == L for el in out)
    return out


def build(ctx, sk, elems, hidden=False, seed=0, plant=()):
    return np.stack([H.noise_ciphertext(ctx, sk, el, hidden, seed + k, plant) for k, el in enumerate(elems)])


@functools.lru_cache(maxsize=None)
def sweep(name):
    """The bare constant sweep of a preset: (all elements, their budgets [n][L]; the decodable values spread again, their
    decodings [n'][L][N]) -- every case checked to be what its kind says."""
    prm, ctx, sk = setup(name)
    cases = H.boundary_values(prm.Q, reduced=name in BIG)
    for c in cases:
        H.check_boundary_case(prm.Q, *c)
    kinds = [c[0] for c in cases]
    assert kinds.count("half") == 4 and kinds.count("tie") >= 5 * (len({c[1] for c in cases}) - 3)
    vals = [c[2] for c in cases]
    elems = spread(vals, prm.L)
    good = spread([v for v in vals if H.expected_budget(ctx, [v])[0] > 0], prm.L)
    return dict(elems=elems, enc=build(ctx, sk, elems), budget=np.array([H.expected_budget(ctx, el) for el in elems]),
                good=good, good_enc=build(ctx, sk, good), good_budget=np.array([H.expected_budget(ctx, el) for el in good]),
                decode={k: H.expected_decode(ctx, el) for k, el in enumerate(good)})


def half_values(Qs):
    """(values whose budget is spent, values that decode) around floor(Q / 2) and around the last row that decodes"""
    Q, tb = H.enc_modulus(Qs), H.noise_tb(Qs)
    h = (Q - 1) // 2
    spent = [h, -h, h - 1, -(h - 1), 1 << (tb - 2), -(1 << (tb - 2)), (1 << (tb - 2)) + 1, -(1 << (tb - 2)) - 1]
    good = [(1 << (tb - 2)) - 1, -((1 << (tb - 2)) - 1), 1 << (tb - 3), -(1 << (tb - 3)), (1 << (tb - 2)) - 2, 2 - (1 << (tb - 2))]
    return spent, good


@functools.lru_cache(maxsize=None)
def hidden_sample(name):
    """A sample of the sweep under a uniform c1: every fifth value, the values around floor(Q / 2) and the last rows, with
    c1 s = Q_j - 1 and c0 = Q_j - 1 planted at the first and last two coefficients."""
    prm, ctx, sk = setup(name)
    vals = [c[2] for c in H.boundary_values(prm.Q)]
    spent, good = half_values(prm.Q)
    pick = list(dict.fromkeys(vals[::5] + spent + good))
    elems = spread(pick, prm.L)
    plant = (0, 1, prm.N_enc - 2, prm.N_enc - 1)
    budget = np.array([H.expected_budget(ctx, el) for el in elems])
    ok = [k for k in range(len(elems)) if budget[k].min() > 0]
    assert len(ok) >= len(elems) // 2 and len(ok) < len(elems)
    return dict(elems=elems, enc=build(ctx, sk, elems, True, 500, plant), budget=budget, ok=ok,
                decode={k: H.expected_decode(ctx, elems[k]) for k in ok})


def peak_positions(n):
    T = enc_threads(n.bit_length() - 1)
    assert n % T == 0 and n // T >= 8  # several coefficients per thread: T - 1 and T are the ends of two strides
    return [0, 1, 63, 64, T - 1, T, n // 2, n - 1]


@functools.lru_cache(maxsize=None)
def peaks(name):
    """General polynomials with one peak: element e has its peak |v| = 2^b + {0, 1, -1} (b: the reduced rows in turn; capped
    at (Q - 1) / 2; the last two elements: 2^(tb - 2) - 1, budget 1, and 2^(tb - 2), none) at position e % 8 of
    peak_positions, of alternating sign, and every other coefficient random with exactly one bit less (low 40 bits random,
    both signs).  Every fifth element is hidden.  Limb i of an element takes the polynomial of element e + 3 i, so the
    limbs differ in peak, position and budget."""
    prm, ctx, sk = setup(name)
    n, tb, Qfull = prm.N_enc, H.noise_tb(prm.Q), H.enc_modulus(prm.Q)
    rows = sorted({c[1] for c in H.boundary_values(prm.Q, reduced=True) if c[1] is not None})
    pos = peak_positions(n)
    count = 40
    assert len(rows) <= count - 2 and rows[-1] == tb - 1
    last = {count - 2: (1 << (tb - 2)) - 1, count - 1: 1 << (tb - 2)}
    rng = np.random.RandomState(17)
    polys, res = [], []
    for e in range(count):
        b = rows[e % len(rows)]
        peak = last.get(e, min((1 << b) + (0, 1, -1)[(e + e // len(rows)) % 3], (Qfull - 1) // 2))
        bits = peak.bit_length()
        sign = np.where(rng.randint(0, 2, size=n) == 1, -1, 1).astype(object)
        if bits >= 2:  # magnitudes in [2^(bits - 2), 2^(bits - 1)): exactly bits - 1 bits
            low = rng.randint(0, 1 << min(40, bits - 2), size=n, dtype=np.int64).astype(object) if bits > 2 else np.zeros(n, dtype=object)
            v = sign * ((1 << (bits - 2)) + low)
        else:
            v = np.zeros(n, dtype=object)
        x = pos[e % len(pos)]
        v[x] = peak if (e // len(pos) + e) % 2 == 0 else -peak
        assert all(abs(int(c)).bit_length() == bits - 1 for c in np.delete(v, x)) and abs(int(v[x])).bit_length() == bits
        polys.append(v)
        res.append(H.poly_residues(ctx, v))
    idx = [[(e + 3 * i) % count for i in range(prm.L)] for e in range(count)]
    elems = [[polys[k] for k in el] for el in idx]
    enc = np.stack([H.noise_ciphertext(ctx, sk, elems[e], e % 5 == 0, 900 + e, (0, n - 1) if e % 5 == 0 else (), [res[k] for k in idx[e]])
                    for e in range(count)])
    budget = np.array([H.expected_budget(ctx, el) for el in elems])
    ok = [e for e in range(count) if budget[e].min() > 0]
    assert len(ok) >= count // 2 and {e % len(pos) for e in ok} == set(range(len(pos)))
    assert {0, 1} <= set(budget.reshape(-1)) and budget[count - 2, 0] == 1 and budget[count - 1, 0] == 0
    return dict(enc=enc, budget=budget, ok=ok, decode={e: H.expected_decode(ctx, elems[e]) for e in ok})


def guard_batch(name, spent_at):
    """48 good elements (constants and their negatives, hidden) in which the (element, limb) pairs of spent_at carry
    |v| = 2^(tb - 2), the smallest magnitude without budget; the other limbs of those elements keep theirs."""
    prm, ctx, sk = setup(name)
    tb = H.noise_tb(prm.Q)
    elems = [[(-1) ** (e + i) * ((1 << ((5 * e + 11 * i) % (tb - 2))) + e) for i in range(prm.L)] for e in range(48)]
    for e, i in spent_at:
        elems[e][i] = (-1) ** e * (1 << (tb - 2))
    budget = np.array([H.expected_budget(ctx, el) for el in elems])
    assert {(int(e), int(i)) for e, i in np.argwhere(budget == 0)} == set(spent_at)
    return elems, build(ctx, sk, elems, True, 700), np.stack([H.expected_decode(ctx, el) for el in elems])


# ---- CPU: the oracle against the Python expectation (pins the builders, and the oracle's centring) -----------------------
def oracle_agrees(ctx, sk, enc, budget, decode):
    """enc [n] elements; budget [n][L]; decode: {element: [L][N]} for every element with budget in all limbs (None: the
    guard's verdict only)"""
    for k in range(len(enc)):
        assert ctx.noise_budget(sk, enc[k]) == list(budget[k]), (k, ctx.noise_budget(sk, enc[k]), budget[k])
        ring, bad = ctx.enc_decode_checked(sk, enc[k])
        if budget[k].min() > 0:
            assert bad == -1, (k, bad, budget[k])
            if decode is not None:
                assert (ring == decode[k]).all() and (ctx.enc_decode(sk, enc[k]) == decode[k]).all(), k
        else:
            assert ring is None and bad == int(np.flatnonzero(budget[k] == 0)[0]), (k, bad, budget[k])


@pytest.mark.parametrize("name", SMALL + ["C2"])
def test_oracle_agrees_on_the_constant_sweep(name):
    """noise_budget, enc_decode and enc_decode_checked of the CPU oracle on every value of the sweep (C2: the reduced
    rows), every limb: the budget, the first spent limb, and v mod q_i in every slot."""
    prm, ctx, sk = setup(name)
    s = sweep(name)
    assert len(s["elems"]) >= (6 * H.noise_tb(prm.Q) - 10 if name in SMALL else 60)
    oracle_agrees(ctx, sk, s["enc"], s["budget"], None)  # budgets and the guard
    assert s["good_budget"].min() > 0
    oracle_agrees(ctx, sk, s["good_enc"], s["good_budget"], s["decode"])
    # the unguarded decode centres the spent values as well: v mod q_i whatever the budget
    for k in range(0, len(s["elems"]), 1 if name in SMALL else 4):
        assert (ctx.enc_decode(sk, s["enc"][k]) == H.expected_decode(ctx, s["elems"][k])).all(), k


@pytest.mark.parametrize("name", SMALL)
def test_oracle_agrees_on_the_hidden_sample(name):
    prm, ctx, sk = setup(name)
    h = hidden_sample(name)
    for j, Qj in enumerate(prm.Q):  # the planted words: c0 = Q_j - 1 at coefficients 1 and n - 1 of every ciphertext
        assert (h["enc"][:, :, 0, j, [1, prm.N_enc - 1]] == np.uint64(Qj - 1)).all() and h["enc"][:, :, 1, j].all()
    oracle_agrees(ctx, sk, h["enc"], h["budget"], h["decode"])


def test_oracle_agrees_on_the_peaked_polynomials():
    """the general polynomials of the peak test on C2 (8192 coefficients, two limbs): budget and decoding"""
    prm, ctx, sk = setup("C2")
    p = peaks("C2")
    sample = [e for e in range(len(p["enc"])) if e % 3 == 0]  # every third element: all eight positions, bare and hidden
    oracle_agrees(ctx, sk, p["enc"][sample], p["budget"][sample], {k: p["decode"][e] for k, e in enumerate(sample) if e in p["decode"]})


def test_half_values_are_what_they_claim():
    for name in SMALL + BIG:
        prm, ctx, _ = setup(name)
        Q, tb = H.enc_modulus(prm.Q), H.noise_tb(prm.Q)
        spent, good = half_values(prm.Q)
        assert all(H.expected_budget(ctx, [v]) == [0] for v in spent)
        assert all(H.expected_budget(ctx, [v]) == [1] for v in good)
        assert max(abs(v) for v in spent) == (Q - 1) // 2 and len(set(spent + good)) == 14
        for v in spent[:4]:
            H.check_boundary_case(prm.Q, "half", None, v)
        for v in spent[4:6] + good[:2]:
            H.check_boundary_case(prm.Q, "tie", tb - 2, v)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
_DEV = {}


def device(name):
    from ringsnark_amd.device import Device
    if name not in _DEV:
        _DEV[name] = Device(P.preset(name))
    return _DEV[name]


def profiled(dev, kernel, fn):
    """fn() with the profile on; asserts that `kernel` (and not its twin of the other arithmetic) ran"""
    dev.set_profiling(True)
    try:
        dev.profile_read()
        out = fn()
        names = {k["name"] for k in dev.profile_read()}
    finally:
        dev.set_profiling(False)
    assert {k for k in names if k.startswith("crt_decode_kernel")} == {kernel}, names
    assert {k for k in names if k.startswith("decrypt_dot_kernel")} == {kernel.replace("crt_decode", "decrypt_dot")}, names
    return out


def device_agrees(name, enc, budget, decode):
    """rs_enc_noise_budget on all of enc, rs_enc_decode on the elements of `decode` ({element: [L][N]})"""
    from ringsnark_amd.device import to_host
    dev = device(name)
    _, _, sk = setup(name)
    dsk, denc = dev.put(sk), dev.put(enc)
    got = profiled(dev, KERNEL[name], lambda: dev.enc_noise_budget(dsk, denc))
    bad = np.argwhere(got != budget)
    assert not len(bad), "%s: %d budgets differ, first (element, limb) %s: %d, expected %d" % (
        name, len(bad), tuple(bad[0]), got[tuple(bad[0])], budget[tuple(bad[0])])
    ok = sorted(decode)
    if not ok:
        return
    import torch
    sub = denc[torch.tensor(ok, device=denc.device)].contiguous()
    dec = to_host(profiled(dev, KERNEL[name], lambda: dev.enc_decode(dsk, sub)))
    for k, e in enumerate(ok):
        assert (dec[k] == decode[e]).all(), "%s: the decoding of element %d differs at (limb, slot) %s" % (name, e, tuple(np.argwhere(dec[k] != decode[e])[0]))


def refused(dev, dsk, denc, count):
    """rs_enc_decode on a batch that has a spent element: (status, message, what it wrote)"""
    from ringsnark_amd.device import _ptr, to_host
    out = dev.ring_empty(count)
    out.fill_(-1)
    rc = dev.lib.rs_enc_decode(dev.h, _ptr(dsk), _ptr(denc), count, _ptr(out), dev.stream())
    return rc, dev.lib.rs_last_error().decode(), to_host(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_every_threshold_row(name):
    """The whole bare constant sweep in one batch: the budget of every (element, limb) -- each row b decides for |v| = 2^b - 1,
    2^b, 2^b + 1 of either sign, each limb of an element holds another value -- and, for the values with budget left,
    v mod q_i in every slot of every limb."""
    s = sweep(name)
    device_agrees(name, s["enc"], s["budget"], {})
    device_agrees(name, s["good_enc"], s["good_budget"], s["decode"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_half_boundary_and_last_decodable_row(name):
    """floor(Q / 2), its negative and their neighbours have no budget; +-(2^(tb - 2) - 1) (budget 1, the largest that
    decodes) and +-2^(tb - 3) decode to v mod q_i with the right sign; |v| = 2^(tb - 2) is refused."""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm, ctx, sk = setup(name)
    dev = device(name)
    tb = H.noise_tb(prm.Q)
    spent, good = half_values(prm.Q)
    elems = spread(spent + good, prm.L)
    budget = np.array([H.expected_budget(ctx, el) for el in elems])
    assert (budget[:len(spent), 0] == 0).all() and (budget[len(spent):, 0] > 0).all()
    gelems = spread(good, prm.L)
    enc = build(ctx, sk, elems)
    device_agrees(name, enc, budget, {})
    device_agrees(name, build(ctx, sk, gelems), np.array([H.expected_budget(ctx, el) for el in gelems]),
                  {k: H.expected_decode(ctx, el) for k, el in enumerate(gelems)})
    # The sign of floor(Q / 2) itself (positive: the residue is not ABOVE it) and of its neighbours shows only in what a
    # refused call has written -- every decoding, csrc/encoding.hip decode_impl -- since none of them has budget: v mod q_i,
    # as the unguarded decode of the oracle gives (test_oracle_agrees_on_the_constant_sweep).
    dsk = dev.put(sk)
    rc, msg, out = refused(dev, dsk, dev.put(enc), len(elems))
    assert rc == _lib.RS_ERR_NOISE and msg.endswith("ciphertext #0 has remaining noise budget 0 <= 0 (element 0 of the batch)"), msg
    for k, el in enumerate(elems):
        assert (out[k] == H.expected_decode(ctx, el)).all(), (k, el)
    # one element, as the verifier sees one: limb L - 1 at 2^(tb - 2) - 1 decodes, at 2^(tb - 2) it is refused by name
    for sign in (1, -1):
        el = [1 << (tb - 3)] * (prm.L - 1) + [sign * ((1 << (tb - 2)) - 1)]
        assert H.expected_budget(ctx, el)[-1] == 1
        assert (to_host(dev.enc_decode(dsk, dev.put(H.noise_ciphertext(ctx, sk, el, False, 0)))) == H.expected_decode(ctx, el)).all()
        el[-1] = sign * (1 << (tb - 2))
        assert H.expected_budget(ctx, el)[-1] == 0
        with pytest.raises(_lib.RsError) as ei:
            dev.enc_decode(dsk, dev.put(H.noise_ciphertext(ctx, sk, el, False, 0)))
        assert ei.value.code == _lib.RS_ERR_NOISE and str(ei.value).endswith("ciphertext #%d has remaining noise budget 0 <= 0" % (prm.L - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_hidden_form(name):
    """the same expectations with the product c1 s taking part, and words at Q_j - 1 in c0 and in c1 s"""
    h = hidden_sample(name)
    device_agrees(name, h["enc"], h["budget"], h["decode"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIG)
def test_peak_position_and_reduction(name):
    """One coefficient above all others by one bit, at the first and last coefficients, either side of a wavefront and of a
    thread's stride (T - 1, T), at n / 2: the per-thread maximum over strided coefficients and the workgroup's atomicMax
    must find it wherever it is; the decoding is that of the whole polynomial."""
    p = peaks(name)
    device_agrees(name, p["enc"], p["budget"], p["decode"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_guard_names_the_first_spent_element_and_writes_the_others(name):
    from ringsnark_amd import _lib
    prm, ctx, sk = setup(name)
    dev = device(name)
    dsk, last = dev.put(sk), prm.L - 1
    for spent_at, first in ((((37, last),), (37, last)), (((37, last), (12, 0)), (12, 0)), (((41, 0), (37, last), (47, last)), (37, last))):
        elems, enc, decode = guard_batch(name, spent_at)
        rc, msg, out = profiled(dev, KERNEL[name], lambda: refused(dev, dsk, dev.put(enc), len(elems)))
        assert rc == _lib.RS_ERR_NOISE
        assert msg.endswith("ciphertext #%d has remaining noise budget 0 <= 0 (element %d of the batch)" % (first[1], first[0])), msg
        others = [e for e in range(len(elems)) if e not in {e for e, _ in spent_at}]
        assert (out[others] == decode[others]).all()
        got = dev.enc_noise_budget(dsk, dev.put(enc))
        assert {(int(e), int(i)) for e, i in np.argwhere(got == 0)} == set(spent_at)


# ---- through the verifiers -------------------------------------------------------------------------------------------------
def add_noise(ctx, sk, elem, bits, pos):
    """elem [L][2][K][N_enc] + NTT(t E) on c0, E one coefficient at `pos` (limb i: pos + i), t = q_i: the plaintext is
    unchanged and the noise of limb i has exactly bits[i] bits.  The element's own noise must be below 2^(min(bits) - 4):
    asserted with the oracle's budget; the result's, in every limb, as well."""
    Q, tb, n = H.enc_modulus(ctx.Q), H.noise_tb(ctx.Q), ctx.N_enc
    have = [tb - 1 - b for b in ctx.noise_budget(sk, elem)]
    out = elem.copy()
    for i, t in enumerate(ctx.q):
        assert have[i] <= bits[i] - 4 and bits[i] <= tb - 1
        # about 1.5 2^(bits - 1): own noise moves it by less than an eighth of 2^(bits - 1); capped under (Q - 1) / 2
        target = min(3 << (bits[i] - 2), (Q - 1) // 2 - (1 << (bits[i] - 4)))
        tE = target // t * t
        assert (1 << (bits[i] - 1)) + (1 << (bits[i] - 4)) <= tE <= min(1 << bits[i], (Q - 1) // 2) - (1 << (bits[i] - 4)), (i, bits[i])
        for j, Qj in enumerate(ctx.Q):
            E = np.zeros(n, dtype=np.uint64)
            E[(pos + i) % n] = tE % Qj
            out[i, 0, j] = ((out[i, 0, j].astype(object) + H._ntt(n.bit_length() - 1, Qj).fwd(E).astype(object)) % Qj).astype(np.uint64)
    assert ctx.noise_budget(sk, out) == [tb - b - 1 for b in bits]
    return out


def verifier_inputs(scheme):
    from tests import test_verify as TV
    c = TV.g16_case("toy", 6) if scheme == "groth16" else TV.rin_case("toy49", 9, False)
    ctx, sk = c["ctx"], c["vk"]["sk"]
    tb = H.noise_tb(ctx.Q)
    n_el = len(c["proof"])
    # every element with one bit of budget in every limb: still a proof
    one_bit = np.stack([add_noise(ctx, sk, c["proof"][k], [tb - 2] * ctx.L, 5 + k) for k in range(n_el)])
    for k in range(n_el):
        assert (ctx.enc_decode(sk, one_bit[k]) == ctx.enc_decode(sk, c["proof"][k])).all()
    # one limb of one element a bit further: spent
    spent = {}
    for k, limb in ((0, ctx.L - 1), (n_el - 1, 0)):
        bits = [tb - 2] * ctx.L
        bits[limb] = tb - 1
        p = one_bit.copy()
        p[k] = add_noise(ctx, sk, c["proof"][k], bits, 9)
        spent[(k, limb)] = p
    return c, one_bit, spent


def test_verifier_inputs_on_the_cpu():
    """budget 1 everywhere / 0 in the chosen limb (asserted by add_noise with the oracle), plaintext unchanged"""
    for scheme in ("groth16", "rinocchio"):
        c, one_bit, spent = verifier_inputs(scheme)
        ctx, sk = c["ctx"], c["vk"]["sk"]
        for (k, limb), p in spent.items():
            assert ctx.enc_decode_checked(sk, p[k]) == (None, limb)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_verifier_accepts_one_bit_of_budget_and_refuses_none(scheme):
    from ringsnark_amd import _lib
    c, one_bit, spent = verifier_inputs(scheme)
    prm, cs = c["prm"], c["cs"]
    dev = device(prm.name)
    dcs = dev.r1cs(cs)
    dvk = (dev.groth16_vk if scheme == "groth16" else dev.rinocchio_vk)(dcs, c["vk"])
    verify = dev.groth16_verify if scheme == "groth16" else dev.rinocchio_verify
    primary = dev.put(c["asg"][: cs.n_inputs])
    empty = [0] * len(one_bit)
    assert verify(dvk, primary, dev.put(c["proof"]), empty).accepted
    got = dev.enc_noise_budget(dev.put(c["vk"]["sk"]), dev.put(one_bit))
    assert (got == 1).all()
    assert profiled(dev, KERNEL[prm.name], lambda: verify(dvk, primary, dev.put(one_bit), empty)).accepted
    for (k, limb), p in spent.items():
        with pytest.raises(_lib.RsError) as ei:
            verify(dvk, primary, dev.put(p), empty)
        assert ei.value.code == _lib.RS_ERR_NOISE
        assert "ciphertext #%d has remaining noise budget 0 <= 0 (element %d of the batch)" % (limb, k) in str(ei.value)
    dvk.close()


# ---- the encode side: the centred lift at its boundary ---------------------------------------------------------------------
LIFT_PRESETS = ["toy49", "toy50", "toy60"]  # FP64 (center) and integer (lift_centered) arithmetic
LIFT_PER_C = 12
M64 = (1 << 64) - 1


def splitmix_at(seed, idx):
    """draw number idx (from 1) of the oracle's splitmix64 stream `seed`"""
    z = (seed + idx * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ternary_error(seed, k, limb, n):
    """e [n] with noise polynomial = centred plaintext + t e, of element k, limb `limb` of enc_encode(.., seed): the
    ciphertext is c0 = -(a s + t e') + plaintext with e'_x = draw x + 1 of the limb's stream mod 3, minus 1 (oracle/rs_oracle.c),
    so e = -e'"""
    stream = ((seed * 65537 + k) * 1315423911 + limb + 1) & M64
    return [1 - splitmix_at(stream, x + 1) % 3 for x in range(n)]


@functools.lru_cache(maxsize=None)
def lift_case(name):
    """Rows whose plaintext has coefficient 0 equal to c, 12 elements for each c in 0, 1, (t - 1) / 2, (t + 1) / 2, t - 1 per
    limb (element k: c number k // 12).  With N slots of N_enc a row of equal slots s encodes to a polynomial whose
    coefficient 0 is s N / N_enc (the inverse transform's coefficient 0 is the mean of all N_enc slots, the others zero), so
    s = c N_enc / N mod t; with N == N_enc that is the constant polynomial c.  The seed is the first whose ternary error has
    e_0 = -1 on some element at c = (t - 1) / 2 and e_0 = +1 on some element at c = (t + 1) / 2, in every limb: there a lift
    with another convention leaves the range centred(c) + t {-1, 0, 1}."""
    prm, ctx, _ = setup(name)
    sk = ctx.keygen(3)
    cs = [[0, 1, (t - 1) // 2, (t + 1) // 2, t - 1] for t in ctx.q]
    count = 5 * LIFT_PER_C
    rings = np.empty((count, ctx.L, ctx.N), dtype=np.uint64)
    for k in range(count):
        for i, t in enumerate(ctx.q):
            rings[k, i] = cs[i][k // LIFT_PER_C] * (ctx.N_enc // ctx.N) % t
            assert int(ctx.batch_encode(i, rings[k, i])[0]) == cs[i][k // LIFT_PER_C]

    def e0(seed, c_idx, limb):
        return {ternary_error(seed, k, limb, 1)[0] for k in range(c_idx * LIFT_PER_C, (c_idx + 1) * LIFT_PER_C)}

    seed = next(s for s in range(1, 200) if all(-1 in e0(s, 2, i) and 1 in e0(s, 3, i) for i in range(ctx.L)))
    return ctx, sk, rings, cs, seed


def compose_centred(ctx, res):
    """res [K][n] residues -> the n centred integers mod Q they compose to (plain CRT in Python integers)"""
    Q = H.enc_modulus(ctx.Q)
    acc = np.zeros(res.shape[1], dtype=object)
    for j, Qj in enumerate(ctx.Q):
        M = Q // Qj
        acc = acc + res[j].astype(object) * (M * pow(M, -1, Qj))
    return [H.centred(int(x), Q) for x in acc]


@pytest.mark.parametrize("name", LIFT_PRESETS)
def test_oracle_lift_is_the_centred_one_at_its_boundary(name):
    """The noise polynomial c0 + c1 s of every oracle encoding of lift_case, composed and centred in Python integers, is
    centred(plain_x) + t e_x with e the ternary error of the element's stream and centred(p) = p - t from p = (t + 1) / 2 on
    (SEAL's rule): coefficient 0 is centred(c) + t e_0."""
    ctx, sk, rings, cs, seed = lift_case(name)
    n = ctx.N_enc
    enc = ctx.enc_encode(sk, rings, seed)
    seen = set()
    for k in range(len(rings)):
        for i, t in enumerate(ctx.q):
            res = np.stack([H._ntt(n.bit_length() - 1, Qj).inv(((enc[k, i, 0, j].astype(object) + enc[k, i, 1, j].astype(object) * sk[j].astype(object)) % Qj).astype(np.uint64))
                            for j, Qj in enumerate(ctx.Q)])
            v = compose_centred(ctx, res)
            e = ternary_error(seed, k, i, n)
            plain = [int(p) for p in ctx.batch_encode(i, rings[k, i])]
            c = cs[i][k // LIFT_PER_C]
            assert plain[0] == c and v[0] == (c if c <= (t - 1) // 2 else c - t) + t * e[0], (k, i, c, v[0], e[0])
            assert v == [(p if p <= (t - 1) // 2 else p - t) + t * ex for p, ex in zip(plain, e)], (k, i)
            seen.add((i, k // LIFT_PER_C, e[0]))
    for i in range(ctx.L):
        assert (i, 2, -1) in seen and (i, 3, 1) in seen  # (t - 1) / 2 - t and -(t - 1) / 2 + t occur: the two ends of the range


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIFT_PRESETS)
def test_lift_boundary_on_the_device(name):
    """rs_enc_encode and rs_enc_encode_linear (one term) on the rows of lift_case: the oracle's bytes"""
    from ringsnark_amd.device import to_host
    ctx, sk, rings, cs, seed = lift_case(name)
    dev = device(name)
    exp = ctx.enc_encode(sk, rings, seed)
    dsk, drings = dev.put(sk), dev.put(rings)
    assert (to_host(dev.enc_encode(dsk, drings, seed)) == exp).all()
    assert (to_host(dev.enc_encode_linear(dsk, [drings], seed)) == exp).all()
    assert (to_host(dev.enc_decode(dsk, dev.put(exp))) == rings).all()
