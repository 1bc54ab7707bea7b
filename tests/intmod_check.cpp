// Host-side exactness check of ringsnark_amd/csrc/intmod.hpp (Montgomery arithmetic, primes 2^50 <= p < 2^62) against
// 128-bit integer arithmetic.  The same header is compiled for gfx950, where mulhi64 is __umul64hi: an integer
// instruction sequence with the same result.  The moduli constants are built as the library builds them (host_math.hpp).
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "../ringsnark_amd/csrc/host_math.hpp"
#include "../ringsnark_amd/csrc/intmod.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;
static uint64_t sm(uint64_t &s) { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static long long fails = 0;
static void expect(bool c, const char *what, uint64_t p, uint64_t a, uint64_t b) {
  if (!c) { if (fails < 10) fprintf(stderr, "FAIL %s p=%llu a=%llu b=%llu\n", what, (unsigned long long)p, (unsigned long long)a, (unsigned long long)b); fails++; }
}
static uint64_t imod(i128 v, uint64_t p) { i128 r = v % (i128)p; if (r < 0) r += p; return (uint64_t)r; }

struct Checker {
  uint64_t p, rinv;  // rinv = 2^-64 mod p
  rs::ModI m;
  // a * b products: one operand < p, the other < 2^64 (the widest form montmul documents), so a * b < 2^126
  void products(uint64_t a, uint64_t b) const {
    const uint64_t ab = (uint64_t)(((u128)a * b) % p);
    const uint64_t redc = (uint64_t)(((u128)ab * rinv) % p);
    expect(rs::montmul(a, b, m) == redc, "montmul", p, a, b);
    expect(rs::mulmod_dd(a, b, m) == ab, "mulmod_dd", p, a, b);
    // data x table constant: the constant in Montgomery form, built on the host as the tables are and on the "device" by to_mont
    if (b < p) {
      expect(rs::mulmod(a, rs::host::mont_form(b, p), m) == ab, "mulmod (host constant)", p, a, b);
      if (a < p) expect(rs::mulmod(a, rs::to_mont(b, m), m) == ab, "mulmod (to_mont constant)", p, a, b);
    }
    if (a < p) expect(rs::mulmod(b, rs::host::mont_form(a, p), m) == ab, "mulmod (host constant, swapped)", p, a, b);
  }
  void both_orders(uint64_t a, uint64_t b) const {
    products(a, b);
    products(b, a);
  }
};

int main(int argc, char **argv) {
  std::vector<uint64_t> primes;
  for (int i = 1; i < argc; i++) primes.push_back(strtoull(argv[i], nullptr, 0));
  uint64_t st = 42;
  for (uint64_t p : primes) {
    if (p < (1ull << 50) || p >= (1ull << 62) || !(p & 1)) { fprintf(stderr, "modulus %llu outside [2^50, 2^62)\n", (unsigned long long)p); return 2; }
    const rs::ModI m{p, rs::host::mont_ninv(p), rs::host::mont_r2(p)};
    const uint64_t R = (uint64_t)(((u128)1 << 64) % p);  // 2^64 mod p
    const uint64_t rinv = rs::host::invmod(R, p);
    const Checker ck{p, rinv, m};
    // the constants themselves
    expect(m.ninv * p == ~0ull, "ninv * p == -1 mod 2^64", p, m.ninv, 0);
    expect(m.r2 == (uint64_t)(((u128)R * R) % p), "r2 == 2^128 mod p", p, m.r2, 0);
    expect((uint64_t)(((u128)R * rinv) % p) == 1, "R * R^-1 == 1", p, R, rinv);

    // ---- edge operands, crossed with themselves
    std::vector<uint64_t> edge = {0, 1, 2, p - 1, p - 2, p / 2, p / 2 + 1, R, p - R, rinv};
    for (int s = 1; s < 64 && (1ull << s) < p; s++) edge.push_back(1ull << s);
    for (uint64_t a : edge)
      for (uint64_t b : edge) ck.products(a, b);
    // 2^s * 2^(64-s): the low word of the product is zero (montmul's lo == 0 branch with a nonzero product); valid whenever
    // one factor is below p
    for (int s = 1; s < 64; s++) {
      const uint64_t a = 1ull << s, b = 1ull << (64 - s);
      if (a < p || b < p) ck.products(a, b);
    }
    // the same branch through odd multiples: (2^s * u) * 2^(64-s), u odd, both below p
    for (int s = 3; s < 61; s++)
      for (uint64_t u : {3ull, 5ull, 255ull}) {
        const uint64_t a = (1ull << s) * u, b = 1ull << (64 - s);
        if (a < p && b < p) ck.products(a, b);
      }
    // one operand beyond p, up to 2^64 - 1, the other below p
    for (uint64_t wide : std::vector<uint64_t>{1ull << 63, ~0ull - 1, ~0ull, p, p + 1, 2 * p - 1, 2 * p, 4 * p - 1})
      for (uint64_t b : edge) ck.both_orders(wide, b);

    // ---- random operands
    for (int it = 0; it < 2000000; it++) {
      const uint64_t ra = sm(st), rb = sm(st);
      const uint64_t a = ra % p, b = rb % p;
      ck.products(a, b);
      if ((it & 15) == 0) ck.both_orders(ra, b);  // one operand anywhere below 2^64
      // to_mont / konst_value round trip, and to_mont against the host's table encoding
      const uint64_t am = rs::to_mont(a, m);
      expect(am < p && am == rs::host::mont_form(a, p), "to_mont == a * 2^64 mod p", p, a, am);
      expect(rs::konst_value(am, m) == a, "konst_value(to_mont(a)) == a", p, a, am);
      // additive operations
      expect(rs::addm(a, b, m) == (uint64_t)(((u128)a + b) % p), "addm", p, a, b);
      expect(rs::subm(a, b, m) == imod((i128)a - (i128)b, p), "subm", p, a, b);
      expect(rs::negm(a, m) == imod(-(i128)a, p), "negm", p, a, 0);
      // lifts: a residue mod p centred, then reduced modulo p itself and (below) another prime
      const int64_t la = rs::lift_centered(a, m);
      expect((a > p / 2 ? (i128)a - p : (i128)a) == (i128)la, "lift_centered", p, a, 0);
      expect(rs::lift_residue(la, m) == a, "lift_residue(lift_centered(a)) == a", p, a, 0);
      const int64_t v = (int64_t)(ra >> 1) - (int64_t)(1ull << 62);  // uniform in [-2^62, 2^62)
      expect(rs::lift_residue(v, m) == imod((i128)v, p), "lift_residue", p, (uint64_t)v, 0);
      expect(rs::small_val(ra, m) == ra % p, "small_val", p, ra, 0);
    }

    // ---- additive operations, conversions and lifts at their edges
    for (uint64_t a : {(uint64_t)0, (uint64_t)1, p - 1, p - 2, p / 2, p / 2 + 1}) {
      for (uint64_t b : {(uint64_t)0, (uint64_t)1, p - 1, p - 2, p / 2, p / 2 + 1}) {
        expect(rs::addm(a, b, m) == (uint64_t)(((u128)a + b) % p), "addm edge", p, a, b);
        expect(rs::subm(a, b, m) == imod((i128)a - (i128)b, p), "subm edge", p, a, b);
      }
      expect(rs::negm(a, m) == imod(-(i128)a, p), "negm edge", p, a, 0);
      expect(rs::reduce(a, m) == a && rs::canon(a, m) == a && rs::center(a, m) == a && rs::to_res(a) == a, "identities", p, a, 0);
    }
    for (uint64_t a : edge) {
      const uint64_t am = rs::to_mont(a, m);
      expect(am == rs::host::mont_form(a, p), "to_mont edge", p, a, am);
      expect(rs::konst_value(am, m) == a, "konst_value edge", p, a, am);
      expect(rs::konst_value(a, m) == (uint64_t)(((u128)a * rinv) % p), "konst_value == c * 2^-64", p, a, 0);
    }
    for (uint64_t v : std::vector<uint64_t>{0, 1, 2, 1000003, p - 1, p, p + 1, 2 * p, 2 * p + 1, 1ull << 63, ~0ull})
      expect(rs::small_val(v, m) == v % p, "small_val edge", p, v, 0);
    // lift_centered: (t - 1) / 2 stays, (t + 1) / 2 becomes -(t - 1) / 2
    const uint64_t h = (p - 1) / 2;
    expect(rs::lift_centered(h, m) == (int64_t)h, "lift_centered((t - 1) / 2)", p, h, 0);
    expect(rs::lift_centered(h + 1, m) == -(int64_t)h, "lift_centered((t + 1) / 2)", p, h + 1, 0);
    expect(rs::lift_centered(0, m) == 0 && rs::lift_centered(1, m) == 1 && rs::lift_centered(p - 1, m) == -1, "lift_centered(0, 1, t - 1)", p, 0, 0);
    // lift_residue modulo every prime of the list Q, of the centred lifts modulo this one and of integers up to +-2^62
    for (uint64_t Q : primes) {
      const rs::ModI mq{Q, rs::host::mont_ninv(Q), rs::host::mont_r2(Q)};
      for (uint64_t c : {(uint64_t)0, (uint64_t)1, h - 1, h, h + 1, h + 2, p - 2, p - 1}) {
        const i128 lifted = c > p / 2 ? (i128)c - p : (i128)c;
        expect(rs::lift_residue(rs::lift_centered(c, m), mq) == imod(lifted, Q), "lift_residue(lift_centered(c, t), Q)", p, c, Q);
      }
      const int64_t big = (int64_t)1 << 62, q = (int64_t)Q;
      for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)-1, q - 1, q, q + 1, -q + 1, -q, -q - 1, big - 1, big, -big + 1, -big})
        expect(rs::lift_residue(v, mq) == imod((i128)v, Q), "lift_residue edge", Q, (uint64_t)v, 0);
    }
  }
  if (fails) { fprintf(stderr, "%lld failures\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
