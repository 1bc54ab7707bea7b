"""rs_ring_inv_or_zero (include/ringsnark_amd/inverse.h): the slotwise inverse-or-zero of ring elements, with a numerator
their slotwise quotients, and where the input is zero or not a canonical residue.

CPU (-m "not gpu"): the header and the binding agree, the header compiles alone, the host mirror
ringsnark_amd.r1cs.inv_or_zero against Python integers, its report on constructed inputs, the is-zero and the division
circuits and their host assignments.
GPU (-m gpu): rows and report of the device equal the mirror's word for word and field for field -- the arithmetic is
exact, so equality is the whole test -- on both arithmetics and both regimes of the FP64 product, one and two limbs, with
and without a numerator, on inputs whose outcome does not depend on how the kernel batches, strided in place, on the launch
shapes that select another path (counts around whole pieces, workgroups that take a second piece, the non-temporal stores
of large outputs), and every invalid argument is refused with the output untouched."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ringsnark_amd", "inverse.h")
# FP64 context L = 2, N = 32 (a limb row shorter than a batch); the two regimes of the FP64 product; Montgomery; L = 1
PRESETS = ("toy", "toy49", "toy50", "toy60", "toy54")
FIELDS = ("n_zero", "zero_elem", "zero_limb", "zero_slot", "n_bad", "bad_elem", "bad_limb", "bad_slot", "bad_x", "bad_num")
CLEAN = (0,) * 10
SENTINEL = 0xA5A5A5A5A5A5A5A5
PIECE_PAIRS = 2048  # csrc/inverse.hip INV_PIECE: slot pairs of ONE limb in a piece
MAX_BLOCKS = 2048  # csrc/inverse.hip rs_ring_inv_or_zero: the bounded grid


def fields(r):
    return tuple(int(getattr(r, f)) for f in FIELDS)


def qcol(prm):
    return np.array(prm.q, dtype=np.uint64).reshape(1, prm.L, 1)


def random_x(prm, count, seed, zeros=True):
    """[count][L][N] canonical residues, none zero but single planted ones."""
    rng = np.random.RandomState(seed)
    x = np.stack([rng.randint(1, p, size=(count, prm.N), dtype=np.uint64) for p in prm.q], axis=1)
    if zeros:
        x[0, 0, 0] = 0
        x[count - 1, prm.L - 1, prm.N - 1] = 0
        x[count // 2, 0, 5] = 0
    return np.ascontiguousarray(x)


def batching_independent_x(prm):
    """The elements whose outcome cannot depend on how a kernel groups words into batches, then random ones."""
    N, L = prm.N, prm.L
    q = qcol(prm)[0]  # [L][1]
    one = np.ones((L, N), dtype=np.uint64)
    rnd = random_x(prm, 4, 77, zeros=False)
    even, odd, ends, limb0 = rnd[0].copy(), rnd[1].copy(), rnd[2].copy(), rnd[3].copy()
    even[:, 0::2] = 0
    odd[:, 1::2] = 0
    ends[:, 0] = ends[:, N - 1] = 0
    limb0[0, 3] = limb0[0, N - 2] = 0  # zero in limb 0 and (L > 1) non-zero in limb 1 at the same slot
    two_half = np.where(np.arange(N) % 2 == 0, np.uint64(2) * one, (q + np.uint64(1)) // np.uint64(2) * one)
    elems = [np.zeros((L, N), dtype=np.uint64), even, odd, ends, limb0, one, (q - np.uint64(1)) * one, two_half]
    return np.ascontiguousarray(np.concatenate([np.stack(elems), random_x(prm, 3, 78)]))


def pow_ref(x, prm, num=None):
    """pow(v, q - 2, q) word by word (0 for 0), times num."""
    out = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        p = prm.q[idx[-2]]
        v = pow(int(x[idx]), p - 2, p)
        out[idx] = v if num is None else v * int(num[idx]) % p
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_inverse_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.INVERSE_SIGNATURES) == {"rs_ring_inv_or_zero"}
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 113
    members = re.search(r"typedef struct rs_inv_report \{(.*?)\}", code, flags=re.S).group(1)
    declared = [n for decl in members.split(";") for n in re.findall(r"\b([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert declared == [k for k, _ in _lib.InvReport._fields_] == list(FIELDS) == list(R.InvReport._fields)
    assert C.sizeof(_lib.InvReport) == 64


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_inverse_h_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no compiler")
    src = tmp_path / ("only." + ("c" if lang == "c" else "cpp"))
    src.write_text("#include <ringsnark_amd/inverse.h>\nint main(void) { rs_inv_report r; r.n_bad = 0; return (int)r.n_bad + (int)sizeof(&rs_ring_inv_or_zero) * 0; }\n")
    r = subprocess.run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", PRESETS)
def test_mirror_against_python_integers(name):
    prm = P.preset(name)
    x = batching_independent_x(prm)
    num = random_x(prm, x.shape[0], 5)
    out, rep = R.inv_or_zero(x, prm.q)
    assert out.shape == x.shape and out.dtype == np.uint64 and rep.clean
    assert (out == pow_ref(x, prm)).all()
    assert rep.n_zero == int((x == 0).sum()) and (rep.zero_elem, rep.zero_limb, rep.zero_slot) == (0, 0, 0)
    quo, qrep = R.inv_or_zero(x, prm.q, num=num)
    assert (quo == pow_ref(x, prm, num)).all() and fields(qrep) == fields(rep)
    ind, _ = R.inv_or_zero(x, prm.q, num=x)
    assert (ind == (x != 0)).all()  # num = x: 1 where non-zero, 0 where zero
    one, rep1 = R.inv_or_zero(x[4], prm.q)
    assert one.shape == x[4].shape and (one == out[4]).all()
    assert fields(rep1) == (2, 0, 0, 3) + (0,) * 6
    assert (out[5] == 1).all() and (out[6] == x[6]).all()  # 1 and q - 1 are their own inverses
    assert (out[7][:, 0::2] == x[7][:, 1::2]).all() and (out[7][:, 1::2] == 2).all()  # 2 and (q + 1) / 2 are each other's


def constructed_inputs(prm):
    """{case: (x [3][L][N], num or None, the expected report)} -- the constructed inputs of the CPU and the GPU tests."""
    N, L, q = prm.N, prm.L, prm.q
    base = random_x(prm, 3, 31, zeros=False)
    num = random_x(prm, 3, 32, zeros=False)
    out = {}
    x = base.copy()
    x[1, L - 1, 7] = 0
    out["one_zero"] = (x, None, (1, 1, L - 1, 7) + (0,) * 6)
    x = base.copy()  # zeros in two elements, one limb each: element 2's has the lower limb*N + slot, element 1's is the first
    x[2, 0, 3] = 0
    x[1, L - 1, N - 1] = 0
    out["zeros_in_two_elements"] = (x, None, (2, 1, L - 1, N - 1) + (0,) * 6)
    x = base.copy()
    x[1, L - 1, 9] = q[L - 1]
    x[2, 0, 1] = 0
    out["word_equal_to_q"] = (x, None, (1, 2, 0, 1, 1, 1, L - 1, 9, q[L - 1], 0))
    x = base.copy()  # far above every modulus, the FP64 conversion's range included
    x[0, 0, 2] = (1 << 64) - 1
    x[2, L - 1, 0] = 1 << 63
    out["word_far_above_q"] = (x, None, (0, 0, 0, 0, 2, 0, 0, 2, (1 << 64) - 1, 0))
    x, n = base.copy(), num.copy()  # a bad numerator over a zero: bad, not zero
    x[1, 0, 4] = 0
    n[1, 0, 4] = q[0]
    n[2, L - 1, 6] = q[L - 1] + 1
    x[0, 0, 8] = 0
    out["bad_numerator"] = (x, n, (1, 0, 0, 8, 2, 1, 0, 4, 0, q[0]))
    if L > 1 and q[0] < q[1]:
        x = base.copy()
        x[1, 1, 9] = q[0]  # a canonical residue of limb 1
        out["q0_in_limb_1"] = (x, None, CLEAN)
    if L > 1 and q[0] > q[1]:
        x = base.copy()
        x[1, 0, 9] = q[1]  # a canonical residue of limb 0
        out["q1_in_limb_0"] = (x, None, CLEAN)
    return out


@pytest.mark.parametrize("name", PRESETS)
def test_mirror_report_on_constructed_inputs(name):
    prm = P.preset(name)
    cases = constructed_inputs(prm)
    assert prm.L == 1 or "q0_in_limb_1" in cases or "q1_in_limb_0" in cases
    for case, (x, num, exp) in cases.items():
        out, rep = R.inv_or_zero(x, prm.q, num=num)
        assert fields(rep) == exp, case
        assert rep.clean == (exp[4] == 0)
        bad = (x >= qcol(prm)) | (False if num is None else num >= qcol(prm))
        assert (out[bad | (x == 0)] == 0).all()
        ok = ~bad & (x != 0)
        assert (out[ok] == pow_ref(np.where(ok, x, 0), prm, None if num is None else np.where(ok, num, 0))[ok]).all(), case


def test_circuits_against_rows_written_by_hand():
    q = P.preset("toy").q
    m1 = q[0] - 1

    def rows_of(cs):
        out = {}
        for name in "abc":
            rp, col, coeff = cs.mats[name]
            out[name] = [[(int(col[e]), int(coeff[0, e])) for e in range(int(rp[i]), int(rp[i + 1]))] for i in range(cs.m)]
        return out

    cs = R.is_zero_r1cs(q, 2)  # one = 1; block 0 = x 2, inv 3, z 4; block 1 = 5, 6, 7
    assert (cs.m, cs.n_vars, cs.n_inputs) == (4, 7, 1) and cs.poly_table is None
    assert rows_of(cs) == {"a": [[(2, 1)], [(2, 1)], [(5, 1)], [(5, 1)]], "b": [[(3, 1)], [(4, 1)], [(6, 1)], [(7, 1)]],
                           "c": [[(1, 1), (4, m1)], [], [(1, 1), (7, m1)], []]}
    cs = R.division_r1cs(q, 2)  # block 0 = a 2, b 3, binv 4, y 5; block 1 = 6, 7, 8, 9
    assert (cs.m, cs.n_vars, cs.n_inputs) == (4, 9, 1) and cs.poly_table is None
    assert rows_of(cs) == {"a": [[(3, 1)], [(5, 1)], [(7, 1)], [(9, 1)]], "b": [[(4, 1)], [(3, 1)], [(8, 1)], [(7, 1)]],
                           "c": [[(1, 1)], [(2, 1)], [(1, 1)], [(6, 1)]]}


@pytest.mark.parametrize("name", ("toy", "toy60", "toy54"))
def test_host_assignments_satisfy_their_circuits(name):
    prm = P.preset(name)
    count = 2
    xs = random_x(prm, count, 3)
    xs[1, :, 4] = 0
    asg = R.is_zero_assignment(xs, prm.q)
    cs = R.is_zero_r1cs(prm.q, count)
    assert asg.shape == (cs.n_vars, prm.L, prm.N) and (asg[0] == 1).all() and (asg[1::3] == xs).all()
    assert (asg[3::3] == (xs == 0)).all()
    assert R.is_satisfied(cs, asg, prm.q).satisfied
    # z = 0 at a zero slot of x_1: x * inv = 0 there, one - z = 1
    bad = asg.copy()
    bad[3 + 3, prm.L - 1, 4] = 0
    chk = R.is_satisfied(cs, bad, prm.q)
    assert (chk.n_violated, chk.first_row, chk.first_limb, chk.first_slot, chk.a, chk.b, chk.c) == (1, 2, prm.L - 1, 4, 0, 0, 1)
    # inv = 0 at a non-zero slot of x_0
    bad = asg.copy()
    bad[2, 0, 9] = 0
    chk = R.is_satisfied(cs, bad, prm.q)
    assert (chk.n_violated, chk.first_row, chk.first_limb, chk.first_slot, chk.a, chk.b, chk.c) == (1, 0, 0, 9, int(xs[0, 0, 9]), 0, 1)
    # the solver's view: z from one, x and inv through the c side
    given = [0] + [1 + 3 * p for p in range(count)] + [2 + 3 * p for p in range(count)]
    solved = R.solve(cs, given, np.where(np.isin(np.arange(cs.n_vars), given)[:, None, None], asg, np.uint64(SENTINEL)), prm.q)
    assert (solved == asg).all()

    a, b = random_x(prm, count, 4), random_x(prm, count, 5, zeros=False)
    dasg = R.division_assignment(a, b, prm.q)
    dcs = R.division_r1cs(prm.q, count)
    assert dasg.shape == (dcs.n_vars, prm.L, prm.N) and (dasg[1::4] == a).all() and (dasg[2::4] == b).all()
    assert R.is_satisfied(dcs, dasg, prm.q).satisfied
    b[1, 0, 6] = 0  # b with a zero slot: no binv exists there
    chk = R.is_satisfied(dcs, R.division_assignment(a, b, prm.q), prm.q)
    # y = 0 there as well, so y * b = a fails too unless a is zero there
    assert (chk.first_row, chk.first_limb, chk.first_slot, chk.a, chk.b, chk.c) == (2, 0, 6, 0, 0, 1) and chk.n_violated == 2


# ---- GPU -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device(name):
    from ringsnark_amd.device import Device
    return Device(P.preset(name))


def run(dev, x, num=None, **kw):
    from ringsnark_amd.device import to_host
    out, rep = dev.ring_inv_or_zero(dev.put(x), None if num is None else dev.put(num), **kw)
    return to_host(out), rep


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_batching_independent_inputs_equal_the_mirror(name):
    from ringsnark_amd.device import to_host
    prm, dev = P.preset(name), device(name)
    x = batching_independent_x(prm)
    num = random_x(prm, x.shape[0], 6)
    for what, n in (("no numerator", None), ("numerator", num), ("num = x", x)):
        exp, exp_rep = R.inv_or_zero(x, prm.q, num=n)
        got, rep = run(dev, x, n)
        assert got.shape == exp.shape and (got == exp).all(), what
        assert fields(rep) == fields(exp_rep) and rep.clean, what
    # num = x as the SAME rows, not a copy
    dx = dev.put(x)
    out, rep = dev.ring_inv_or_zero(dx, dx)
    assert (to_host(out) == (x != 0)).all() and rep.n_zero == int((x == 0).sum())
    # each element alone: another place in its batch, the same words
    exp, _ = R.inv_or_zero(x, prm.q)
    for e in range(x.shape[0]):
        got, rep = run(dev, x[e:e + 1])
        assert (got[0] == exp[e]).all() and rep.n_zero == int((x[e] == 0).sum()), e


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_constructed_inputs_report_equals_the_mirror(name):
    prm, dev = P.preset(name), device(name)
    for case, (x, num, exp_fields) in constructed_inputs(prm).items():
        exp, exp_rep = R.inv_or_zero(x, prm.q, num=num)
        got, rep = run(dev, x, num)
        assert fields(rep) == fields(exp_rep) == exp_fields, (case, fields(rep), exp_fields)
        assert (got == exp).all(), case


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_agrees_with_ring_inv_where_that_succeeds(name):
    from ringsnark_amd.device import to_host
    prm, dev = P.preset(name), device(name)
    x = random_x(prm, 5, 91, zeros=False)
    got, rep = run(dev, x)
    assert fields(rep) == CLEAN
    assert (got == to_host(dev.ring_inv(dev.put(x)))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_strided_in_place_touches_the_output_rows_only(name):
    from ringsnark_amd.device import to_host
    prm, dev = P.preset(name), device(name)
    count = 3
    xs = random_x(prm, count, 500)
    buf = np.full((1 + 3 * count, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf[0] = 1
    buf[1::3] = xs
    d = dev.put(buf)
    rep = dev.is_zero_fill(d, count)
    exp = buf.copy()
    exp[2::3], exp_rep = R.inv_or_zero(xs, prm.q)
    assert fields(rep) == fields(exp_rep) and rep.n_zero == 3
    assert (to_host(d) == exp).all()

    a, b = random_x(prm, count, 501), random_x(prm, count, 502)
    buf = np.full((1 + 4 * count, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf[0] = 1
    buf[1::4], buf[2::4] = a, b
    d = dev.put(buf)
    rep_binv, rep_y = dev.division_fill(d, count)
    exp = buf.copy()
    exp[3::4], exp_binv = R.inv_or_zero(b, prm.q)
    exp[4::4], exp_y = R.inv_or_zero(b, prm.q, num=a)
    assert fields(rep_binv) == fields(exp_binv) and fields(rep_y) == fields(exp_y)
    assert (to_host(d) == exp).all()
    assert (exp == R.division_assignment(a, b, prm.q)).all()


def per_piece(prm):
    assert PIECE_PAIRS % (prm.N // 2) == 0
    return PIECE_PAIRS // (prm.N // 2)  # elements of a piece


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_counts_around_whole_pieces(name):
    prm, dev = P.preset(name), device(name)
    pp = per_piece(prm)
    for count in (pp - 1, pp, pp + 1, 2 * pp + 1):
        x = random_x(prm, count, count % 1000)
        x[count - 1, 0, prm.N - 3] = prm.q[0]  # one bad word in the last element
        num = random_x(prm, count, 7, zeros=False) if count == pp + 1 else None
        exp, exp_rep = R.inv_or_zero(x, prm.q, num=num)
        assert exp_rep.n_zero == 3 and (exp_rep.n_bad, exp_rep.bad_elem, exp_rep.bad_slot) == (1, count - 1, prm.N - 3)
        got, rep = run(dev, x, num)
        assert fields(rep) == fields(exp_rep), count
        assert (got == exp).all(), count


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,with_num,what", [
    ("toy", 0, False, "the output exactly 64 MiB: non-temporal stores, one piece a workgroup"),
    ("toy", 5, True, "more pieces than workgroups: a second round with a guarded last piece"),
    ("toy60", 5, False, "the same on the Montgomery arithmetic"),
])
def test_large_launch_shapes(name, extra, with_num, what):
    """Too large for the integer mirror: x * out == 1 (num: == num) wherever x != 0 by rs_ring_mul, out == 0 wherever
    x == 0, the report against numpy, and a fixed sample of words against the mirror."""
    from ringsnark_amd.device import to_host
    prm, dev = P.preset(name), device(name)
    count = MAX_BLOCKS // prm.L * per_piece(prm) + extra
    assert (count - extra) * prm.ring_words * 8 == 64 << 20
    rng = np.random.RandomState(12)
    x = np.stack([rng.randint(1, p, size=(count, prm.N), dtype=np.uint64) for p in prm.q], axis=1)
    x[rng.randint(0, 16, size=x.shape) == 0] = 0
    x[0, 0, :4] = 1  # the first zero is not at the first word
    num = np.stack([rng.randint(0, p, size=(count, prm.N), dtype=np.uint64) for p in prm.q], axis=1) if with_num else None
    dx = dev.put(x)
    dnum = None if num is None else dev.put(num)
    out, rep = dev.ring_inv_or_zero(dx, dnum)
    zero = x == 0
    first = int(np.argmax(zero.reshape(-1)))
    assert fields(rep) == (int(zero.sum()), first // prm.ring_words, first % prm.ring_words // prm.N, first % prm.N) + (0,) * 6, what
    prod = to_host(dev.ring_mul(dx, out))
    got = to_host(out)
    assert (got[zero] == 0).all() and (prod[zero] == 0).all(), what
    assert (prod[~zero] == (1 if num is None else num[~zero])).all(), what
    assert (got < qcol(prm)).all()
    sample = np.random.RandomState(13).randint(0, x.size, size=3000)
    sample[:3] = (0, x.size - 1, x.size - prm.N)  # the first word, the last one, the last limb row's first
    sx = x.reshape(-1)[sample].reshape(-1, 1, 1)
    for limb in range(prm.L):
        pick = sample // prm.N % prm.L == limb
        exp, _ = R.inv_or_zero(sx[pick], [prm.q[limb]], num=None if num is None else num.reshape(-1)[sample].reshape(-1, 1, 1)[pick])
        assert (got.reshape(-1)[sample][pick] == exp.reshape(-1)).all(), (what, limb)


@pytest.mark.gpu
def test_invalid_arguments_write_nothing():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm, dev = P.preset("toy"), device("toy")
    count, S = 3, prm.ring_words
    x = dev.put(random_x(prm, count, 1))
    num = dev.put(random_x(prm, count, 2))
    out = dev.put(np.full((4 * count, prm.L, prm.N), SENTINEL, dtype=np.uint64))
    px, pn, po = x.data_ptr(), num.data_ptr(), out.data_ptr()
    rep = _lib.InvReport()

    def call(d_x, x_stride, d_num, num_stride, n, d_out, out_stride, report=True, ctx=True):
        return dev.lib.rs_ring_inv_or_zero(dev.h if ctx else None, C.c_void_p(d_x), x_stride, C.c_void_p(d_num), num_stride, n,
                                           C.c_void_p(d_out), out_stride, C.byref(rep) if report else None, dev.stream())

    row = S * 8
    refused = {
        "null d_x": ((None, 1, None, 1, count, po, 1), "null"),
        "null d_out": ((px, 1, None, 1, count, None, 1), "null"),
        "x_stride = 0": ((px, 0, None, 1, count, po, 1), "x_stride must be at least 1"),
        "out_stride = 0": ((px, 1, None, 1, count, po, 0), "out_stride must be at least 1"),
        "num_stride = 0": ((px, 1, pn, 0, count, po, 1), "num_stride must be at least 1"),
        "misaligned x": ((px + 8, 1, None, 1, count - 1, po, 1), "16-byte aligned"),
        "misaligned num": ((px, 1, pn + 8, 1, count - 1, po, 1), "16-byte aligned"),
        "misaligned out": ((px, 1, None, 1, count, po + 8, 1), "16-byte aligned"),
        "extent beyond 2^60 words": ((px, 1 << 30, None, 1, (1 << 24) + 1, po, 1), "more than 2^60 words"),
        "out extent beyond 2^60 words": ((px, 1, None, 1, (1 << 24) + 1, po, 1 << 30), "more than 2^60 words"),
        # in place with x taken at stride 1: x of element 1 is the output row of element 0
        "x row 1 is an output row": ((po, 1, None, 1, count, po + row, 3), "x element 1 shares a word with output element 0"),
        "x row 0 is an output row": ((po, 3, None, 1, count, po, 3), "x element 0 shares a word with output element 0"),
        # half a row into the output row of element 2
        "x straddles an output row": ((po + 6 * row + row // 2, 1, None, 1, count, po, 3), "x element 0 shares a word with output element 2"),
        "num row is an output row": ((px, 1, po + 3 * row, 3, count, po, 3), "num element 0 shares a word with output element 1"),
    }
    for what, (args, msg) in refused.items():
        assert call(*args) == _lib.RS_ERR_INVALID, what
        assert msg in dev.lib.rs_last_error().decode(), (what, dev.lib.rs_last_error())
    assert call(px, 1, None, 1, count, po, 1, ctx=False) == _lib.RS_ERR_INVALID
    dev.sync()
    assert (to_host(out) == SENTINEL).all()
    # num_stride does not matter without a numerator
    scratch = dev.ring_empty(count)
    assert call(px, 1, None, 0, count, scratch.data_ptr(), 1) == _lib.RS_OK and rep.n_zero == 3
    # count = 0: nothing to do, whatever else is passed
    rep.n_zero = rep.n_bad = 77
    assert call(None, 0, None, 0, 0, None, 0) == _lib.RS_OK and rep.n_zero == 0 and rep.n_bad == 0
    assert call(None, 0, None, 0, 0, None, 0, report=False) == _lib.RS_OK
    # the in-place layouts themselves are legal: x, inv, z blocks; x rows and num rows that are the same rows
    buf = np.full((3 * count, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf[0::3] = to_host(x)
    d = dev.put(buf)
    assert call(d.data_ptr(), 3, d.data_ptr(), 3, count, d.data_ptr() + row, 3) == _lib.RS_OK and rep.n_zero == 3 and rep.n_bad == 0
    dev.sync()
    got = to_host(d)
    assert (got[1::3] == (buf[0::3] != 0)).all() and (got[0::3] == buf[0::3]).all() and (got[2::3] == SENTINEL).all()
    assert (to_host(out) == SENTINEL).all()


@pytest.mark.gpu
def test_without_a_report_the_rows_are_the_same_after_a_sync():
    from ringsnark_amd.device import to_host
    prm, dev = P.preset("toy"), device("toy")
    x = random_x(prm, 130, 9)
    x[7, 1, 2] = prm.q[1]  # bad input changes nothing about how the rows are made
    num = random_x(prm, 130, 10)
    for n in (None, num):
        exp, _ = R.inv_or_zero(x, prm.q, num=n)
        out, rep = dev.ring_inv_or_zero(dev.put(x), None if n is None else dev.put(n), want_report=False)
        assert rep is None
        dev.sync()
        assert (to_host(out) == exp).all()
