"""Exactness of the Montgomery integer arithmetic of every context with a modulus >= 2^50 (ringsnark_amd/csrc/intmod.hpp),
checked on the host against 128-bit integers: the products on the edges that random residues almost never reach (a zero
low word, operands 0, 1, p - 1, the r >= p boundary, one operand up to 2^64 - 1), 2 * 10^6 random pairs per prime, the
additive operations, the Montgomery-form round trip and the lifts (tests/intmod_check.cpp)."""
import os
import subprocess
import tempfile

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _next_prime(n, step):
    n |= 1
    while not P.is_prime(n):
        n += step
    return n


def test_intmod_exact_against_int128():
    primes = set()
    for name in ("toy54", "toy60", "micro60", "C5"):
        prm = P.preset(name)
        primes.update(p for p in prm.q + prm.Q if p >= 1 << 50)
    assert len(primes) >= 8 and {p.bit_length() for p in primes} == {54, 59, 60}, sorted(primes)
    lo, hi = _next_prime((1 << 50) + 1, 2), _next_prime((1 << 62) - 1, -2)  # the ends of the range the contexts accept
    assert 1 << 50 < lo < (1 << 50) + 1000 and (1 << 62) - 1000 < hi < 1 << 62
    primes.update((lo, hi))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "intmod_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "intmod_check.cpp"), "-o", exe])
        out = subprocess.run([exe] + [str(p) for p in sorted(primes)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == "ok"
