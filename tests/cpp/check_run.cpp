// check_run.cpp -- run-time check of ringsnark::amd::is_satisfied (include/ringsnark_amd/r1cs_check.hpp) against librs_hip.so:
// plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: check_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// A six-constraint chain x_i * x_{i+1} = x_{i+2} (x_0, x_1 primary) written as R1csCsr by hand: satisfied by the
// forward-solved assignment, not satisfied after one wire is changed in one slot -- and the report says where.
#include <cstdio>
#include <cstdlib>
#include <random>

#include <ringsnark_amd/r1cs_check.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

int main(int argc, char **argv) {
  int a = 1;
  Params p;
  p.N = std::atoi(argv[a++]);
  p.L = std::atoi(argv[a++]);
  for (int i = 0; i < p.L; i++) p.q.push_back(std::strtoull(argv[a++], nullptr, 10));
  p.N_enc = std::atoi(argv[a++]);
  p.K = std::atoi(argv[a++]);
  for (int i = 0; i < p.K; i++) p.Q.push_back(std::strtoull(argv[a++], nullptr, 10));
  EXPECT(a == argc);
  Context::set_context(p);

  const size_t m = 6;
  R1csCsr csr;
  csr.m = m;
  csr.n_vars = m + 2;
  csr.n_inputs = 2;
  for (int w = 0; w < 3; w++) {
    csr.row_ptr[w].push_back(0);
    for (size_t i = 0; i < m; i++) {
      csr.col[w].push_back((uint32_t)(i + 1 + w));  // a: x_i, b: x_{i+1}, c: x_{i+2}; index 0 is the constant one
      csr.row_ptr[w].push_back((uint32_t)(i + 1));
    }
    csr.coeff[w].assign((size_t)p.L * m, 1);  // [L][nnz]
  }
  const DeviceR1cs cs(csr);

  std::mt19937_64 g(11);
  std::vector<RingElem> x;
  for (int k = 0; k < 2; k++) {
    std::vector<uint64_t> w(Context::ring_words());
    for (int i = 0; i < p.L; i++)
      for (int s = 0; s < p.N; s++) w[(size_t)i * p.N + s] = 1 + g() % (p.q[i] - 1);  // non-zero: so is every product
    x.emplace_back(std::move(w));
  }
  for (size_t i = 0; i < m; i++) x.push_back(x[i] * x[i + 1]);
  const std::vector<RingElem> primary(x.begin(), x.begin() + 2);
  std::vector<RingElem> aux(x.begin() + 2, x.end());

  r1cs_violation v{};
  EXPECT(is_satisfied(cs, primary, aux));
  EXPECT(is_satisfied(cs, primary, aux, &v));
  EXPECT(v.n_violated == 0 && v.constraint == m && v.limb == 0 && v.slot == 0 && v.a == 0 && v.b == 0 && v.c == 0);

  // x_4 is c of constraint 2, b of constraint 3 and a of constraint 4: one more in one slot of the last limb breaks those three
  const int limb = p.L - 1, slot = 3;
  const size_t at = (size_t)limb * p.N + slot;
  std::vector<uint64_t> w4 = x[4].get_poly();
  w4[at] = (w4[at] + 1) % p.q[limb];
  aux[2] = RingElem(std::move(w4));
  EXPECT(!is_satisfied(cs, primary, aux));
  EXPECT(!is_satisfied(cs, primary, aux, &v));
  EXPECT(v.n_violated == 3 && v.constraint == 2 && v.limb == limb && v.slot == slot);
  EXPECT(v.a == x[2].get_poly()[at] && v.b == x[3].get_poly()[at] && v.c == aux[2].get_poly()[at]);

  try {
    is_satisfied(cs, primary, std::vector<RingElem>(aux.begin(), aux.end() - 1));
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()) == "assignment does not match the constraint system");
  }

  if (fails) {
    std::fprintf(stderr, "check_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("check_run: OK\n");
  return 0;
}
