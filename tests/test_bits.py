"""rs_ring_bit_decompose (include/ringsnark_amd/bits.h): the bit rows of ring elements whose slots hold one integer below
2^nbits in every limb, and where the input is not of that form.

CPU (-m "not gpu"): the header and the binding agree, the header compiles alone, the host mirror
ringsnark_amd.r1cs.bit_decompose against Python integers, its report on constructed bad inputs.
GPU (-m gpu): rows and report of the device equal the mirror's word for word and field for field -- integers only, so
equality is the whole test -- on both arithmetics, one and two limbs, strided in place, on the launch shapes that select
another path (more elements than a grid dimension holds, the non-temporal stores of large outputs, counts around whole
pieces, workgroups that take a second piece), and every invalid argument is refused with the output untouched."""
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
HEADER = os.path.join(ROOT, "include", "ringsnark_amd", "bits.h")
PRESETS = ("toy", "toy49", "toy50", "toy60", "toy54")  # FP64 context L = 2; N = 64; primes just below 2^50; integer context; L = 1 (no second limb to compare)
FIELDS = ("n_bad", "first_elem", "first_limb", "first_slot", "word", "value")
SENTINEL = 0xA5A5A5A5A5A5A5A5
PIECE_PAIRS = 2048  # csrc/bits.hip BITS_PIECE: slot pairs of a piece


def fields(r):
    return tuple(int(getattr(r, f)) for f in FIELDS)


def nbits_cases(name):
    return (1, 8, R.max_nbits(P.preset(name).q))


def valid_x(prm, count, nbits, seed):
    """[count][L][N]: random values below 2^nbits, the same word in every limb; 0, 2^nbits - 1 planted in fixed slots."""
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 1 << nbits, size=(count, prm.N), dtype=np.uint64)
    v[0, 0] = 0
    v[0, 1] = (1 << nbits) - 1
    v[count - 1, prm.N - 1] = (1 << nbits) - 1
    v[count - 1, prm.N - 2] = 0
    return np.ascontiguousarray(np.repeat(v[:, None, :], prm.L, axis=1))


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_bits_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.BITS_SIGNATURES) == {"rs_ring_bit_decompose"}
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 109
    members = re.search(r"typedef struct rs_bits_report \{(.*?)\}", code, flags=re.S).group(1)
    declared = [n for decl in members.split(";") for n in re.findall(r"\b([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert declared == [k for k, _ in _lib.BitsReport._fields_] == list(FIELDS)
    assert C.sizeof(_lib.BitsReport) == 40


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_bits_h_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no compiler")
    src = tmp_path / ("only." + ("c" if lang == "c" else "cpp"))
    src.write_text("#include <ringsnark_amd/bits.h>\nint main(void) { rs_bits_report r; r.n_bad = 0; return (int)r.n_bad + (int)sizeof(&rs_ring_bit_decompose) * 0; }\n")
    r = subprocess.run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", PRESETS)
def test_mirror_against_python_integers(name):
    prm = P.preset(name)
    assert R.max_nbits(prm.q) == min(p.bit_length() - 1 for p in prm.q)
    for nbits in nbits_cases(name):
        assert all((1 << nbits) <= p for p in prm.q)  # every nbits-bit value is a canonical residue
        x = valid_x(prm, 3, nbits, 7 + nbits)
        bits, rep = R.bit_decompose(x, nbits, prm.q)
        assert bits.shape == (3, nbits, prm.L, prm.N) and bits.dtype == np.uint64
        assert fields(rep) == (0, 0, 0, 0, 0, 0) and rep.clean
        for e in range(3):
            for s in range(prm.N):
                v = int(x[e, 0, s])
                for l in range(prm.L):
                    assert [int(b) for b in bits[e, :, l, s]] == [(v >> k) & 1 for k in range(nbits)]
                assert sum(int(bits[e, k, 0, s]) << k for k in range(nbits)) == v
        one, rep1 = R.bit_decompose(x[1], nbits, prm.q)
        assert (one == bits[1]).all() and rep1.clean
    for bad_nbits in (0, R.max_nbits(prm.q) + 1):
        with pytest.raises(AssertionError, match="floor"):
            R.bit_decompose(valid_x(prm, 1, 1, 0), bad_nbits, prm.q)


def bad_inputs(prm, nbits):
    """{case: x [3][L][N]} -- the constructed bad inputs of the CPU and the GPU tests."""
    N, L = prm.N, prm.L
    base = valid_x(prm, 3, nbits, 31 + nbits)
    out = {}
    x = base.copy()
    x[1, :, 5] = 1 << nbits  # the smallest value that does not fit, in every limb: limb 0 alone is bad
    out["two_pow_nbits"] = x
    x = base.copy()
    x[1, 0, 6] = prm.q[0] - 1  # the largest canonical residue of limb 0, there only: every limb of the slot is bad
    out["q0_minus_1"] = x
    if L > 1:
        x = base.copy()
        x[2, 1, 9] ^= 1  # limb 1 off by one
        out["limb1_off_by_one"] = x
    x = base.copy()  # two bad positions, the one later in launch order first in report order
    x[2, :, 3] = 1 << nbits
    if L > 1:
        x[0, 1, N - 1] ^= 1
    else:
        x[0, 0, N - 1] = 1 << nbits
    out["two_positions"] = x
    return out


@pytest.mark.parametrize("name", PRESETS)
def test_mirror_report_on_constructed_bad_inputs(name):
    prm = P.preset(name)
    N, L = prm.N, prm.L
    for nbits in nbits_cases(name):
        cases = bad_inputs(prm, nbits)
        top = 1 << nbits
        exp = {"two_pow_nbits": (1, 1, 0, 5, top, top),
               "q0_minus_1": (L, 1, 0, 6, prm.q[0] - 1, prm.q[0] - 1),
               "two_positions": (2, 0, 1, N - 1, int(cases["two_positions"][0, L - 1, N - 1]), int(cases["two_positions"][0, 0, N - 1]))
               if L > 1 else (2, 0, 0, N - 1, top, top)}
        if L > 1:
            v = int(cases["limb1_off_by_one"][2, 0, 9])
            exp["limb1_off_by_one"] = (1, 2, 1, 9, v ^ 1, v)
        assert set(exp) == set(cases)
        for case, x in cases.items():
            bits, rep = R.bit_decompose(x, nbits, prm.q)
            assert fields(rep) == exp[case], (case, nbits)
            assert not rep.clean
            # the bits of a bad slot are the low nbits bits of the limb-0 word
            assert ((x[:, None, :1, :] >> np.arange(nbits, dtype=np.uint64).reshape(1, nbits, 1, 1)) & np.uint64(1) == bits).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device(name):
    from ringsnark_amd.device import Device
    return Device(P.preset(name))


def decompose(dev, x, nbits, **kw):
    from ringsnark_amd.device import to_host
    out, rep = dev.ring_bit_decompose(dev.put(x), nbits, **kw)
    return to_host(out), rep


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_valid_inputs_equal_the_mirror(name):
    prm, dev = P.preset(name), device(name)
    for nbits in nbits_cases(name):
        for count in (1, 3):
            x = valid_x(prm, count, nbits, 100 * count + nbits)
            exp, exp_rep = R.bit_decompose(x, nbits, prm.q)
            got, rep = decompose(dev, x, nbits)
            assert got.shape == exp.shape and (got == exp).all(), (nbits, count)
            assert fields(rep) == fields(exp_rep) == (0, 0, 0, 0, 0, 0) and bool(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_bad_inputs_report_equals_the_mirror(name):
    prm, dev = P.preset(name), device(name)
    for nbits in nbits_cases(name):
        for case, x in bad_inputs(prm, nbits).items():
            exp, exp_rep = R.bit_decompose(x, nbits, prm.q)
            got, rep = decompose(dev, x, nbits)
            assert exp_rep.n_bad >= 1 and not rep
            assert fields(rep) == fields(exp_rep), (case, nbits, fields(rep), fields(exp_rep))
            assert (got == exp).all(), (case, nbits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
def test_strided_in_place_touches_the_bit_rows_only(name):
    from ringsnark_amd.device import to_host
    prm, dev = P.preset(name), device(name)
    for nbits in nbits_cases(name):
        count, w = 3, nbits + 1
        x = valid_x(prm, count, nbits, 500 + nbits)
        buf = np.full((1 + count * w + 1, prm.L, prm.N), SENTINEL, dtype=np.uint64)  # a row before and a row after the blocks
        blocks = buf[1:1 + count * w].reshape(count, w, prm.L, prm.N)
        blocks[:, nbits] = x
        d = dev.put(buf)
        _, rep = dev.ring_bit_decompose(d[1 + nbits:], nbits, out=d[1:], x_stride=w, bits_stride=w)
        got = to_host(d)
        exp = buf.copy()
        exp[1:1 + count * w].reshape(count, w, prm.L, prm.N)[:, :nbits] = R.bit_decompose(x, nbits, prm.q)[0]
        assert fields(rep) == (0, 0, 0, 0, 0, 0)
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()
        assert (got[1:1 + count * w].reshape(count, w, prm.L, prm.N)[:, nbits] == x).all()
        assert (got == exp).all(), nbits


def per_piece(prm):
    assert PIECE_PAIRS % (prm.N // 2) == 0
    return PIECE_PAIRS // (prm.N // 2)  # elements of a piece


@pytest.mark.gpu
@pytest.mark.parametrize("count,nbits,what", [
    (65537, 2, "more elements than one grid dimension holds"),
    (16387, 8, "the output just over 64 MiB: the path of large outputs"),
    (127, 8, "just below one piece"), (129, 8, "just above one piece"), (257, 3, "just above two pieces"),
    (2048 * 128 + 5, 1, "more pieces than workgroups: a second round"),
])
def test_launch_shapes(count, nbits, what):
    prm, dev = P.preset("toy"), device("toy")
    assert per_piece(prm) == 128
    if "64 MiB" in what:
        assert (count - 3) * nbits * prm.ring_words * 8 == 64 << 20 and count * nbits * prm.ring_words * 8 > 64 << 20
    x = valid_x(prm, count, nbits, count % 1000)
    x[count - 1, 0, prm.N - 3] = 1 << nbits  # one bad word in the last element
    exp, exp_rep = R.bit_decompose(x, nbits, prm.q)
    assert fields(exp_rep) == (prm.L, count - 1, 0, prm.N - 3, 1 << nbits, 1 << nbits)
    got, rep = decompose(dev, x, nbits)
    assert fields(rep) == fields(exp_rep), what
    assert (got == exp).all(), what


@pytest.mark.gpu
def test_invalid_arguments_write_nothing():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm, dev = P.preset("toy"), device("toy")
    nbits, count, S = 8, 3, prm.ring_words
    top = R.max_nbits(prm.q)
    x = dev.put(valid_x(prm, count, nbits, 1))
    rows = 2 * count * (top + 2)
    out = dev.put(np.full((rows, prm.L, prm.N), SENTINEL, dtype=np.uint64))
    px, po = x.data_ptr(), out.data_ptr()
    rep = _lib.BitsReport()

    def call(d_x, x_stride, n, nb, d_bits, bits_stride, report=True):
        return dev.lib.rs_ring_bit_decompose(dev.h, C.c_void_p(d_x), x_stride, n, nb, C.c_void_p(d_bits), bits_stride,
                                             C.byref(rep) if report else None, dev.stream())

    w = nbits + 1
    refused = {
        "nbits = 0": ((px, 1, count, 0, po, nbits), "floor(log2 q_i)"),
        "nbits above the limit": ((px, 1, count, top + 1, po, top + 1), "floor(log2 q_i) = %d" % top),
        "bits_stride < nbits": ((px, 1, count, nbits, po, nbits - 1), "bits_stride must be at least nbits = 8"),
        "x_stride = 0": ((px, 0, count, nbits, po, nbits), "x_stride must be at least 1"),
        "null d_x": ((None, 1, count, nbits, po, nbits), "null"),
        "null d_bits": ((px, 1, count, nbits, None, nbits), "null"),
        "misaligned": ((px + 8, 1, count - 1, nbits, po, nbits), "16-byte aligned"),
        # in place, but the x rows are taken at stride 1: x of element 1 is bit row 0 of element 1
        "x row 1 is a bit row": ((po + nbits * S * 8, 1, count, nbits, po, w), "input element 1 shares a word with the bit rows of element 1"),
        # x is the last bit row of element 0
        "x row 0 is a bit row": ((po + (nbits - 1) * S * 8, w, count, nbits, po, w), "input element 0 shares a word with the bit rows of element 0"),
        # half a row into the bit rows of element 2
        "x straddles a bit row": ((po + (2 * w * S + S // 2) * 8, 1, count, nbits, po, w), "input element 0 shares a word with the bit rows of element 2"),
    }
    for what, (args, msg) in refused.items():
        assert call(*args) == _lib.RS_ERR_INVALID, what
        assert msg in dev.lib.rs_last_error().decode(), (what, dev.lib.rs_last_error())
    dev.sync()
    assert (to_host(out) == SENTINEL).all()
    # count = 0: nothing to do, whatever else is passed
    rep.n_bad = 77
    assert call(None, 0, 0, 0, None, 0) == _lib.RS_OK and rep.n_bad == 0
    assert call(None, 0, 0, 0, None, 0, report=False) == _lib.RS_OK
    # the in-place layout itself is legal: x rows between the blocks of bit rows
    buf = np.full((count * w, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf.reshape(count, w, prm.L, prm.N)[:, nbits] = to_host(x)
    d = dev.put(buf)
    assert call(d.data_ptr() + nbits * S * 8, w, count, nbits, d.data_ptr(), w) == _lib.RS_OK and rep.n_bad == 0
    dev.sync()
    assert (to_host(out) == SENTINEL).all()


@pytest.mark.gpu
def test_without_a_report_the_rows_are_the_same_after_a_sync():
    from ringsnark_amd.device import to_host
    prm, dev = P.preset("toy"), device("toy")
    nbits = 8
    x = valid_x(prm, 130, nbits, 9)
    x[7, 1, 2] ^= 1  # bad input changes nothing about the rows
    exp, _ = R.bit_decompose(x, nbits, prm.q)
    out, rep = dev.ring_bit_decompose(dev.put(x), nbits, want_report=False)
    assert rep is None
    dev.sync()
    assert (to_host(out) == exp).all()
