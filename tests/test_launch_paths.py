"""The launch paths that the operand size or the batch size selects, each against the CPU oracle (integer array equality;
never one device path against another alone).  Needs a real MI355X: run with -m gpu.

Which test reaches which code:

test_ring_ops_on_every_stream_path -- ring_pointwise_kernel<OP, Mod | ModI, NT> (csrc/rs_core.hip) for OP = add, sub, mul, neg,
add_scalar, mul_scalar.  A workgroup moves pieces of 2048 16-byte pairs and a tail loop takes pairs % 2048; the limb of a
word is looked up per access when logN < 12; the grid is capped at 2048 workgroups and operands of 64 MiB or more take the
non-temporal instantiation, so a second grid-stride round exists there only.  RING_SHAPES:
    pieces            toy / toy+int / toy60, 128 elements   two whole pieces, no tail, per-access limb
    pieces+tail       toy / toy+int / toy60, 100 elements   one piece + 1152 pairs in one launch, per-access limb
    full-grid         C2 / C2+int, 1023 elements            2046 pieces = the largest launch that is not non-temporal
    nt+round2         C2 / C2+int, 1100 elements            NT, 2200 pieces: 152 workgroups run a second round, uniform limb
    nt+round2+tail    mid / mid50 / mid60, 8801 elements            NT, 2200 pieces + 512 pairs, per-access limb
add and mul run a second time with dst == a (the C entry point directly) at pieces+tail and nt+round2+tail.

test_enc_add_on_every_stream_path -- enc_add_kernel<NT> (csrc/msm_mac.hpp), the same shape with the prime of a word in place
of the limb; ENC_SHAPES, out of place and with dst == a (the only way include/ringsnark_amd/ring.hpp calls it).

test_ring_inv_second_round_and_late_zero -- ring_inv_kernel (C2) / ring_inv_kernel_int (mid60): more words than the capped
grid covers in one round (4096 x 256), so the stride loop runs twice for some threads; then one zero among the words of
the second round, which must raise RS_ERR_NOT_INVERTIBLE.

test_ring_is_zero_finds_single_words -- ring_nonzero_kernel: 300 elements, three of them with one nonzero word each (word 0,
the last word, a word the block reaches in a later round of its loop).

test_wide_transforms_with_several_polynomials_per_workgroup -- ntt_fwd_wide_kernel / ntt_inv_wide_kernel<LOGN, RED>
(csrc/ntt_wide.hpp) with ntt_wide_grid = 1: 4, 2 or 1 workgroups and 3 * grid + 1 polynomials, so a workgroup runs the
software pipeline (prefetch of polynomial p + grid, flush of the previous one out of the tile, reuse of the tile) three and
four times.  WIDE_CASES lists the <LOGN, RED> instantiations each context reaches, forward and inverse.
test_wide_transforms_at_the_default_grid -- the same kernels at the default knob, 8192 points: 515 polynomials on 512
workgroups.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import _lib
from ringsnark_amd import params as P
from tests import helpers as H
from tests.test_gpu_parity import dev_for, host

pytestmark = pytest.mark.gpu

# contexts that are no preset: name -> make_params arguments
CUSTOM = {
    "mid": (512, [43, 44], 512, [49, 48, 48]),    # 1024 ring words, 6144 encoding words per element; FP64 arithmetic
    "mid50": (512, [50, 50], 512, [50, 50, 50]),  # the same shape on primes just below 2^50, the largest of the FP64 arithmetic
    "mid60": (512, [59, 60], 512, [60, 60, 59]),  # the same shape on the integer arithmetic
    "w12": (4096, [43], 4096, [49, 36]),
    "w13": (8192, [43], 8192, [49, 48]),
    "w14": (16384, [43], 16384, [43, 44]),
    "w14s": (16384, [36], 16384, [43]),           # a 36-bit prime at 16384 points: the inverse transform without reductions
}
_PARAMS, _DEVS = {}, {}


def _base(name):
    return name[:-4] if name.endswith("+int") else name


def _params(name):
    name = _base(name)
    if name not in _PARAMS:
        _PARAMS[name] = P.make_params(*CUSTOM[name], name=name) if name in CUSTOM else P.preset(name)
    return _PARAMS[name]


def _dev(name):
    """The device context of a preset (shared with tests/test_gpu_parity.py; "+int": forced integer arithmetic) or of CUSTOM."""
    if name not in CUSTOM:
        return dev_for(name)
    if name not in _DEVS:
        from ringsnark_amd.device import Device
        _DEVS[name] = Device(_params(name))
    return _DEVS[name]


def _assert_same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got.reshape(-1) != exp.reshape(-1))
        raise AssertionError("%s: %d of %d words differ, the first at word %d, the last at word %d"
                             % (what, bad.size, exp.size, bad[0], bad[-1]))


# ---------------------------------------------------------------------------------------------------------------------
# dyadic streams
# ---------------------------------------------------------------------------------------------------------------------
PIECE = 2048          # 16-byte pairs a workgroup moves at a time (32 KiB)
MAX_GRID = 2048       # workgroups at most
NT_BYTES = 64 << 20   # operands of this size and more: the non-temporal instantiation
SCALARS = (0, 1, 2**40 + 12345, 2**63 + 99)


def _stream_path(pairs, row_words):
    """What a launch of `pairs` 16-byte words does, by the arithmetic of launch_pointwise_arith / enc_add_run and of the
    kernels; row_words: words that share a limb / prime (N / N_enc)."""
    grid = max(1, min((pairs + PIECE - 1) // PIECE, MAX_GRID))
    return dict(pieces=pairs // PIECE, tail=pairs % PIECE, nt=pairs * 16 >= NT_BYTES, second_round=pairs // PIECE > grid,
                per_access=row_words < 4096)


RING_SHAPES = {  # path -> (contexts, elements, what _stream_path must say)
    "pieces": (("toy", "toy+int", "toy60"), 128, dict(pieces=2, tail=0, nt=False, second_round=False, per_access=True)),
    "pieces+tail": (("toy", "toy+int", "toy60"), 100, dict(pieces=1, tail=1152, nt=False, second_round=False, per_access=True)),
    "full-grid": (("C2", "C2+int"), 1023, dict(pieces=2046, tail=0, nt=False, second_round=False, per_access=False)),
    "nt+round2": (("C2", "C2+int"), 1100, dict(pieces=2200, tail=0, nt=True, second_round=True, per_access=False)),
    "nt+round2+tail": (("mid", "mid50", "mid60"), 8801, dict(pieces=2200, tail=512, nt=True, second_round=True, per_access=True)),
}
ENC_SHAPES = {
    "pieces": ((("toy49", 8), ("toy60", 16)), dict(pieces=3, tail=0, nt=False, second_round=False, per_access=True)),
    "pieces+tail": ((("toy49", 7), ("toy60", 14)), dict(pieces=2, tail=1280, nt=False, second_round=False, per_access=True)),
    "nt+round2": ((("C2", 70),), dict(pieces=2240, tail=0, nt=True, second_round=True, per_access=False)),
    "nt+round2+tail": ((("mid", 1501), ("mid50", 1501), ("mid60", 1501)), dict(pieces=2251, tail=1024, nt=True, second_round=True, per_access=True)),
}
IN_PLACE = ("pieces+tail", "nt+round2+tail")
RING_OPS = ("add", "sub", "mul", "neg", "add_scalar", "mul_scalar")
# a shape's operands and an operation's expected results are built once and serve every context on the same moduli: the cases
# of one (path, op) follow each other, and only the operands of the latest shape and the latest results are kept (an
# operand is up to 70 MiB)
RING_CASES = [(path, op, name) for path, (names, _, _) in RING_SHAPES.items() for op in RING_OPS for name in names]
ENC_CASES = [(path, name, count) for path, (cases, _) in ENC_SHAPES.items() for name, count in cases]


def _plant(flat, primes, row_words, boundaries, shift):
    """Writes 0, 1, p - 1, (p - 1) / 2 (p: the modulus of the word) over the four words before and the four words after every
    boundary (a word index; 0 and flat.size: the ends of the operand).  shift = 0 / 1 for the two operands of a binary
    operation: every pair of the four values then meets somewhere."""
    pos = list(dict.fromkeys(w for b in boundaries for w in range(b - 4, b + 4) if 0 <= w < flat.size))
    for k, w in enumerate(pos):
        p = primes[(w // row_words) % len(primes)]
        flat[w] = (0, 1, p - 1, (p - 1) // 2)[(k + shift * (k // 4)) % 4]
    return pos


def _boundaries(words, row_words, n_rows):
    """The ends of the operand, the first and the last piece boundary, the first limb / prime boundary, the first element
    boundary and the last limb / prime boundary."""
    last_piece = (words // 2 // PIECE) * PIECE * 2
    return [0, words, 2 * PIECE, last_piece, row_words, row_words * n_rows, words - row_words]


_RING_IN, _RING_EXP, _ENC = {}, {}, {}


def _ring_inputs(base, count):
    if (base, count) not in _RING_IN:
        if any(c != count for _, c in _RING_IN):
            _RING_IN.clear()
        prm = _params(base)
        ctx = H.oracle_ctx(prm)
        a, b = ctx.random_ring(101, count), ctx.random_ring(102, count)
        bounds = _boundaries(a.size, prm.N, prm.L)
        pos = _plant(a.reshape(-1), prm.q, prm.N, bounds, 0)
        _plant(b.reshape(-1), prm.q, prm.N, bounds, 1)
        assert len(pos) >= 32  # eight groups of four: all sixteen pairs of planted values occur
        _RING_IN[(base, count)] = (ctx, a, b)
    return _RING_IN[(base, count)]


def _ring_expected(base, count, op):
    """[(scalar or None, expected)] from the oracle"""
    if (base, count, op) not in _RING_EXP:
        _RING_EXP.clear()
        ctx, a, b = _ring_inputs(base, count)
        if op in ("add", "sub", "mul"):
            exp = [(None, getattr(ctx, "ring_" + op)(a, b))]
        elif op == "neg":
            exp = [(None, ctx.ring_neg(a))]
        elif op == "add_scalar":  # RingElem + Scalar: the scalar promoted to a polynomial (seal_ring.tcc:265-277), then added
            exp = [(s, ctx.ring_add(a, np.ascontiguousarray(np.broadcast_to(ctx.ring_scalar(s), a.shape)))) for s in SCALARS]
        else:
            exp = [(s, ctx.ring_mul_scalar(a, s)) for s in SCALARS]
        _RING_EXP[(base, count, op)] = exp
    return _RING_EXP[(base, count, op)]


@pytest.mark.parametrize("path,op,name", RING_CASES)
def test_ring_ops_on_every_stream_path(path, op, name):
    from ringsnark_amd.device import _ptr
    _, count, expect = RING_SHAPES[path]
    dev = _dev(name)
    prm = dev.prm
    assert (prm.N, prm.L) == (_params(name).N, _params(name).L)
    pairs = count * prm.ring_words // 2
    assert _stream_path(pairs, prm.N) == expect, (path, name, _stream_path(pairs, prm.N))
    if expect["second_round"]:
        assert pairs > MAX_GRID * PIECE == 4194304
    _, a, b = _ring_inputs(_base(name), count)
    da, db = dev.put(a), dev.put(b)
    for s, exp in _ring_expected(_base(name), count, op):
        if op in ("add", "sub", "mul"):
            got = getattr(dev, "ring_" + op)(da, db)
        elif op == "neg":
            got = dev.ring_neg(da)
        else:
            got = getattr(dev, "ring_" + op)(da, s)
        _assert_same(host(got), exp, "%s %s %s scalar %s" % (path, name, op, s))
        if op in ("add", "mul") and path in IN_PLACE:  # dst == a, as ring.hpp's operators call it
            x = da.clone()
            _lib.check(getattr(dev.lib, "rs_ring_" + op)(dev.h, _ptr(x), _ptr(x), _ptr(db), count, dev.stream()))
            _assert_same(host(x), exp, "%s %s %s in place" % (path, name, op))
    assert (host(da) == a).all() and (host(db) == b).all()  # the operands of the out-of-place calls are untouched


def _enc_case(base, count):
    if (base, count) not in _ENC:
        _ENC.clear()
        prm = _params(base)
        ctx = H.oracle_ctx(prm)
        a, b = ctx.random_enc(103, count), ctx.random_enc(104, count)
        bounds = _boundaries(a.size, prm.N_enc, prm.K)
        pos = _plant(a.reshape(-1), prm.Q, prm.N_enc, bounds, 0)
        _plant(b.reshape(-1), prm.Q, prm.N_enc, bounds, 1)
        assert len(pos) >= 32
        _ENC[(base, count)] = (a, b, np.stack([ctx.enc_add(a[k], b[k]) for k in range(count)]))
    return _ENC[(base, count)]


@pytest.mark.parametrize("path,name,count", ENC_CASES)
def test_enc_add_on_every_stream_path(path, name, count):
    from ringsnark_amd.device import _ptr
    expect = ENC_SHAPES[path][1]
    dev = _dev(name)
    prm = dev.prm
    pairs = count * prm.enc_words // 2
    assert _stream_path(pairs, prm.N_enc) == expect, (path, name, _stream_path(pairs, prm.N_enc))
    if expect["second_round"]:
        assert pairs > MAX_GRID * PIECE == 4194304
    a, b, exp = _enc_case(name, count)
    da, db = dev.put(a), dev.put(b)
    _assert_same(host(dev.enc_add(da, db)), exp, "%s %s enc_add" % (path, name))
    assert (host(da) == a).all() and (host(db) == b).all()
    if path in IN_PLACE:  # EncodingElem::operator+= (ring.hpp): dst == a
        _lib.check(dev.lib.rs_enc_add(dev.h, _ptr(da), _ptr(da), _ptr(db), count, dev.stream()))
        _assert_same(host(da), exp, "%s %s enc_add in place" % (path, name))


# ---------------------------------------------------------------------------------------------------------------------
# ring_inv, ring_is_zero
# ---------------------------------------------------------------------------------------------------------------------
INV_ROUND = 4096 * 256  # words one round of ring_inv_kernel's capped grid covers


@pytest.mark.parametrize("name,count", [("C2", 129), ("mid60", 1025)])
def test_ring_inv_second_round_and_late_zero(name, count):
    from ringsnark_amd._lib import RS_ERR_NOT_INVERTIBLE, RsError
    dev = _dev(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    words = count * prm.ring_words
    assert INV_ROUND < words < 2 * INV_ROUND  # some threads run the stride loop twice, the others once
    a = ctx.random_ring(111, count)
    _plant(a.reshape(-1), prm.q, prm.N, _boundaries(words, prm.N, prm.L) + [INV_ROUND], 0)
    a[a == 0] = 1
    exp, ok = ctx.ring_inv(a)
    assert ok
    _assert_same(host(dev.ring_inv(dev.put(a))), exp, "%s ring_inv" % name)
    z = a.copy()
    at = words - 500
    assert at >= INV_ROUND and words - at <= 1000  # a word of the second round only
    z.reshape(-1)[at] = 0
    with pytest.raises(RsError) as ei:
        dev.ring_inv(dev.put(z))
    assert ei.value.code == RS_ERR_NOT_INVERTIBLE and "not invertible in ring" in str(ei.value)


@pytest.mark.parametrize("name", ["toy", "C2"])
def test_ring_is_zero_finds_single_words(name):
    dev = _dev(name)
    prm = dev.prm
    count, w = 300, prm.ring_words
    later = 4096 + 300 if name == "C2" else w // 2 + 5  # C2: beyond the 256 words a block reads in its first round
    assert later < w - 1 and (name != "C2" or later >= 256)
    a = np.zeros((count, prm.L, prm.N), dtype=np.uint64)
    nonzero = {0: w - 1, 150: later, 299: 0}  # element -> its one nonzero word
    for k, word in nonzero.items():
        a[k].reshape(-1)[word] = 1
    assert dev.ring_is_zero(dev.put(a)) == [k not in nonzero for k in range(count)]


# ---------------------------------------------------------------------------------------------------------------------
# wide transforms
# ---------------------------------------------------------------------------------------------------------------------
WIDE_PER_CU = {12: 4, 13: 2, 14: 1}  # workgroups per unit of ntt_wide_grid (launch_ntt_wide_shape): grid = min(batch, knob * this)


def _fwd_reduces(p, logn):
    """fwd_reduce_mask(p, logn) != 0 (csrc/rs_core.hip): the forward kernel's RED"""
    lim, B = 1125899906842624.0 / float(p), 1.0
    for _ in range(logn):
        if B > lim:
            return True
        B += 0.75
    return False


def _inv_reduces(p, logn):
    """inv_reduce_mask(p, logn) != 0: the inverse kernel's RED"""
    lim, B = 1125899906842624.0 / float(p), 1.0
    for _ in range(logn):
        if 2.0 * B > lim:
            return True
        B = max(2.0 * B, 0.75)
    return False


# context -> (moduli sets, <LOGN, RED> of the forward kernel its primes must reach, of the inverse kernel)
WIDE_CASES = {
    "w12": ("qQ", {(12, True), (12, False)}, {(12, True), (12, False)}),
    "w13": ("qQ", {(13, True), (13, False)}, {(13, True)}),
    "C2": ("qQ", {(13, False)}, {(13, True), (13, False)}),
    "w14": ("qQ", {(14, False)}, {(14, True)}),
    "C5s": ("Q", {(14, True)}, {(14, True)}),  # the data primes
    "w14s": ("q", {(14, False)}, {(14, False)}),
}


def _wide_primes(name):
    prm = _params(name)
    sets = WIDE_CASES[name][0]
    return ([(_lib.RS_MOD_PLAIN, i, p) for i, p in enumerate(prm.q)] if "q" in sets else []) + \
           ([(_lib.RS_MOD_COEFF, j, p) for j, p in enumerate(prm.Q)] if "Q" in sets else [])


def _wide_rows(n, p, count, seed):
    """The seven structured rows of tests/test_gpu_parity.py's _structured_ntt_cases (all p - 1, all (p - 1) / 2, alternating
    0, p - 1, a unit impulse at 0, 1, n / 2 and n - 1), then random rows: `count` rows, every one different."""
    assert count >= 7
    a = np.random.RandomState(seed).randint(0, 2**62, size=(count, n), dtype=np.int64).astype(np.uint64) % np.uint64(p)
    a[:7] = 0
    a[0] = p - 1
    a[1] = (p - 1) // 2
    a[2, 1::2] = p - 1
    for row, pos in zip(range(3, 7), (0, 1, n // 2, n - 1)):
        a[row, pos] = 1
    assert len({r.tobytes() for r in a}) == count
    return a


def _wide_launch(dev, d, modset, idx, inverse):
    """One transform launch that must be the wide kernel's (the profile names the kernel launch_ntt chose)"""
    dev.profile_read()
    dev.ntt(d, modset, idx, inverse=inverse)
    kernels = [(k["name"], k["launches"]) for k in dev.profile_read()]
    assert kernels == [("ntt_inv_wide_kernel" if inverse else "ntt_fwd_wide_kernel", 1)], kernels


def _check_wide(dev, modset, idx, p, rows, what):
    """rows [batch][n] through one forward launch, the inverse of its result, and one inverse launch: every row against the oracle"""
    logn = rows.shape[1].bit_length() - 1
    t = H._ntt(logn, p)
    d = dev.put(rows)
    _wide_launch(dev, d, modset, idx, False)
    got = host(d)
    for b, row in enumerate(rows):
        _assert_same(got[b], t.fwd(row), "%s forward row %d of %d" % (what, b, len(rows)))
    _wide_launch(dev, d, modset, idx, True)
    _assert_same(host(d), rows, "%s inverse of the forward result" % what)
    d = dev.put(rows)
    _wide_launch(dev, d, modset, idx, True)
    got = host(d)
    for b, row in enumerate(rows):
        _assert_same(got[b], t.inv(row), "%s inverse row %d of %d" % (what, b, len(rows)))


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_wide_transforms_with_several_polynomials_per_workgroup(name):
    dev = _dev(name)
    prm = dev.prm
    n, logn = prm.N_enc, prm.N_enc.bit_length() - 1
    primes = _wide_primes(name)
    assert {(logn, _fwd_reduces(p, logn)) for _, _, p in primes} == WIDE_CASES[name][1]
    assert {(logn, _inv_reduces(p, logn)) for _, _, p in primes} == WIDE_CASES[name][2]
    assert _lib.get_tuning("ntt_variant") == 14
    with _lib.tuning(ntt_wide_grid=1):
        grid = _lib.get_tuning("ntt_wide_grid") * WIDE_PER_CU[logn]
        batch = 3 * grid + 1
        assert grid == {12: 4, 13: 2, 14: 1}[logn] and batch > grid  # one workgroup runs four iterations, the others three
        dev.set_profiling(True)
        try:
            for modset, idx, p in primes:
                rows = _wide_rows(n, p, 2 * batch, seed=idx + 10 * modset)  # two launches: the structured rows do not fit one
                for r0 in (0, batch):
                    _check_wide(dev, modset, idx, p, rows[r0:r0 + batch], "%s set %d prime %d rows %d.." % (name, modset, idx, r0))
        finally:
            dev.set_profiling(False)


def test_wide_transforms_at_the_default_grid():
    """8192 points, the 49-bit prime, the default knob: 512 workgroups and 515 polynomials, so three workgroups run twice."""
    dev = _dev("w13")
    prm = dev.prm
    p, batch = prm.Q[0], 515
    assert prm.N_enc == 8192 and p.bit_length() == 49 and _fwd_reduces(p, 13) and _inv_reduces(p, 13)
    grid = _lib.get_tuning("ntt_wide_grid") * WIDE_PER_CU[13]
    assert _lib.get_tuning("ntt_variant") == 14 and grid == 512 and grid < batch < 2 * grid
    dev.set_profiling(True)
    try:
        _check_wide(dev, _lib.RS_MOD_COEFF, 0, p, _wide_rows(8192, p, batch, seed=7), "w13 default grid")
    finally:
        dev.set_profiling(False)
