// solve_run.cpp -- run-time check of ringsnark::amd::solve_plan / solve (include/ringsnark_amd/r1cs_solve.hpp) against
// librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: solve_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// A twelve-constraint wide system written as R1csCsr by a closed formula (tests/test_r1cs_solve_cpp.py builds the same one):
//   (c_i + sum_{k<3} f_ik x_{v_ik}) * x_{i+1} = x_{i+2},   c_i = i % 4 + 1,  v_ik = (7 i + 3 k) % (i + 2),
//   f_ik = (i + k) % 5 - 2, or 1 where that is 0;   x_0[l][s] = (s s + 3 + l) % q_l,  x_1[l][s] = (7 s + 11 + 5 l) % q_l   (0-based variables)
// solved from {x_0, x_1} in every mode, accepted by is_satisfied; prints an FNV-1a digest of the assignment words.
#include <cstdio>
#include <cstdlib>

#include <ringsnark_amd/r1cs_check.hpp>
#include <ringsnark_amd/r1cs_solve.hpp>

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

  const size_t m = 12;
  R1csCsr csr;
  csr.m = m;
  csr.n_vars = m + 2;
  csr.n_inputs = 2;
  std::vector<int64_t> lit[3];  // signed literals; index 0 is the constant one, variable v is column v + 1
  for (int w = 0; w < 3; w++) csr.row_ptr[w].push_back(0);
  for (size_t i = 0; i < m; i++) {
    csr.col[0].push_back(0);
    lit[0].push_back((int64_t)(i % 4) + 1);
    for (size_t k = 0; k < 3; k++) {
      const int64_t f = (int64_t)((i + k) % 5) - 2;
      csr.col[0].push_back((uint32_t)((7 * i + 3 * k) % (i + 2)) + 1);
      lit[0].push_back(f ? f : 1);
    }
    csr.col[1].push_back((uint32_t)(i + 2));
    lit[1].push_back(1);
    csr.col[2].push_back((uint32_t)(i + 3));
    lit[2].push_back(1);
    for (int w = 0; w < 3; w++) csr.row_ptr[w].push_back((uint32_t)csr.col[w].size());
  }
  for (int w = 0; w < 3; w++)  // [L][nnz]: a literal c < 0 is the negation of -c modulo q_l
    for (int l = 0; l < p.L; l++)
      for (const int64_t c : lit[w]) csr.coeff[w].push_back(c < 0 ? p.q[l] - (uint64_t)(-c) % p.q[l] : (uint64_t)c % p.q[l]);
  const DeviceR1cs cs(csr);

  std::vector<RingElem> x(m + 2);  // the unknown wires: default-constructed
  for (int k = 0; k < 2; k++) {
    std::vector<uint64_t> w(Context::ring_words());
    for (int l = 0; l < p.L; l++)
      for (uint64_t s = 0; s < (uint64_t)p.N; s++) w[(size_t)l * p.N + s] = (k == 0 ? s * s + 3 + l : 7 * s + 11 + 5 * l) % p.q[l];
    x[k] = RingElem(std::move(w));
  }
  std::vector<bool> given(m + 2, false);
  given[0] = given[1] = true;
  const solve_plan plan(cs, given);
  const rs_r1cs_solve_info &info = plan.info();
  EXPECT(info.n_given == 2 && info.n_solved == m && info.n_unsolved == 0 && info.first_unsolved == m + 2);
  EXPECT(info.n_levels == m && info.max_width == 1 && info.n_unused == 0 && info.first_blocked == m && info.blocked_reason == 0);
  const std::vector<uint32_t> wires = plan.solved_wires();
  for (size_t i = 0; i < m; i++) EXPECT(wires[i] == i + 2);

  uint64_t digest[3];
  for (int mode = 0; mode < 3; mode++) {
    std::vector<RingElem> full(x);
    const rs_r1cs_solve_stats st = solve(plan, full, mode);
    if (mode == RS_SOLVE_LEVELS) EXPECT(st.level_launches == m && st.walk_launches == 0);
    if (mode == RS_SOLVE_WALK) EXPECT(st.level_launches == 0 && st.walk_launches == 1);
    EXPECT(full[0].get_poly() == x[0].get_poly() && full[1].get_poly() == x[1].get_poly());
    EXPECT(is_satisfied(cs, std::vector<RingElem>(full.begin(), full.begin() + 2), std::vector<RingElem>(full.begin() + 2, full.end())));
    // constraint 0 by the ring operators: (1 - 2 x_0 - x_1 + x_0) * x_1 = x_2
    EXPECT(full[2].get_poly() == ((RingElem(1) - x[0] - x[1]) * x[1]).to_poly().get_poly());
    uint64_t h = 0xcbf29ce484222325ull;
    for (const uint64_t v : flatten(full)) h = (h ^ v) * 0x100000001b3ull;
    digest[mode] = h;
  }
  EXPECT(digest[0] == digest[1] && digest[1] == digest[2]);

  // only x_0 given: the first constraint has an unknown on its b side, nothing can be solved
  given[1] = false;
  const solve_plan partial(cs, given);
  EXPECT(partial.info().n_solved == 0 && partial.info().n_unsolved == m + 1 && partial.info().first_unsolved == 1);
  EXPECT(partial.info().first_blocked == 0 && partial.info().blocked_reason == 1);
  try {
    std::vector<RingElem> full(x);
    solve(partial, full);
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()).find("first unsolved variable 1,") != std::string::npos);
  }
  try {
    std::vector<RingElem> full(x.begin(), x.end() - 1);
    solve(plan, full);
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()) == "assignment does not match the constraint system");
  }

  if (fails) {
    std::fprintf(stderr, "solve_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("solve_run: OK digest %016llx\n", (unsigned long long)digest[0]);
  return 0;
}
