// r1cs_batch_run.cpp -- run-time check of ringsnark::amd::solve_batch / is_satisfied_batch
// (include/ringsnark_amd/r1cs_batch.hpp) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: r1cs_batch_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The twelve-constraint system of solve_run.cpp (tests/test_r1cs_batch_cpp.py builds the same one):
//   (c_i + sum_{k<3} f_ik x_{v_ik}) * x_{i+1} = x_{i+2},   c_i = i % 4 + 1,  v_ik = (7 i + 3 k) % (i + 2),
//   f_ik = (i + k) % 5 - 2, or 1 where that is 0
// and THREE statements, member b given  x_0[l][s] = (s s + 3 + l + 17 b) % q_l,  x_1[l][s] = (7 s + 11 + 5 l + 29 b) % q_l.
// Solved from {x_0, x_1} in one batch in every mode, accepted by is_satisfied_batch, equal to solve() member by member;
// then one word of member 1 is changed and the check must say so for member 1 alone.  Prints an FNV-1a digest per member.
#include <cstdio>
#include <cstdlib>

#include <ringsnark_amd/r1cs_batch.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

static uint64_t digest_of(const std::vector<RingElem> &full) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (const uint64_t v : flatten(full)) h = (h ^ v) * 0x100000001b3ull;
  return h;
}

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

  const size_t m = 12, B = 3;
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

  std::vector<std::vector<RingElem>> x(B, std::vector<RingElem>(m + 2));  // the unknown wires: default-constructed
  for (size_t b = 0; b < B; b++)
    for (int k = 0; k < 2; k++) {
      std::vector<uint64_t> w(Context::ring_words());
      for (int l = 0; l < p.L; l++)
        for (uint64_t s = 0; s < (uint64_t)p.N; s++)
          w[(size_t)l * p.N + s] = (k == 0 ? s * s + 3 + l + 17 * b : 7 * s + 11 + 5 * l + 29 * b) % p.q[l];
      x[b][k] = RingElem(std::move(w));
    }
  std::vector<bool> given(m + 2, false);
  given[0] = given[1] = true;
  const solve_plan plan(cs, given);
  EXPECT(plan.info().n_solved == m && plan.info().n_unsolved == 0);

  // member by member through the single call: what the batch must reproduce
  uint64_t single[B];
  for (size_t b = 0; b < B; b++) {
    std::vector<RingElem> full(x[b]);
    solve(plan, full);
    single[b] = digest_of(full);
  }
  EXPECT(single[0] != single[1] && single[1] != single[2]);

  std::vector<std::vector<RingElem>> solved;
  for (int mode = 0; mode < 3; mode++) {
    std::vector<std::vector<RingElem>> full(x);
    const rs_r1cs_solve_stats st = solve_batch(plan, full, mode);
    if (mode == RS_SOLVE_LEVELS) EXPECT(st.level_launches == m && st.walk_launches == 0);  // of the batch: those of one call
    if (mode == RS_SOLVE_WALK) EXPECT(st.level_launches == 0 && st.walk_launches == 1);
    for (size_t b = 0; b < B; b++) {
      EXPECT(full[b][0].get_poly() == x[b][0].get_poly() && full[b][1].get_poly() == x[b][1].get_poly());
      EXPECT(digest_of(full[b]) == single[b]);
      // constraint 0 by the ring operators: (1 - 2 x_0 - x_1 + x_0) * x_1 = x_2
      EXPECT(full[b][2].get_poly() == ((RingElem(1) - x[b][0] - x[b][1]) * x[b][1]).to_poly().get_poly());
    }
    for (const r1cs_violation &v : is_satisfied_batch(cs, full)) EXPECT(v.n_violated == 0 && v.constraint == m);
    solved = full;
  }

  // one word of member 1 changed: x_5 (0-based), the product of constraint 3, in the last slot of the last limb
  {
    std::vector<std::vector<RingElem>> bad(solved);
    std::vector<uint64_t> w = bad[1][5].get_poly();
    w.back() = (w.back() + 1) % p.q[p.L - 1];
    bad[1][5] = RingElem(std::move(w));
    const std::vector<r1cs_violation> v = is_satisfied_batch(cs, bad);
    EXPECT(v.size() == B && v[0].n_violated == 0 && v[2].n_violated == 0);
    EXPECT(v[1].n_violated >= 1 && v[1].constraint == 3 && v[1].limb == p.L - 1 && v[1].slot == p.N - 1);
    r1cs_violation one{};
    EXPECT(!is_satisfied(cs, std::vector<RingElem>(bad[1].begin(), bad[1].begin() + 2), std::vector<RingElem>(bad[1].begin() + 2, bad[1].end()), &one));
    EXPECT(one.n_violated == v[1].n_violated && one.constraint == v[1].constraint && one.a == v[1].a && one.b == v[1].b && one.c == v[1].c);
  }

  // what the adapter refuses
  try {
    std::vector<std::vector<RingElem>> none;
    solve_batch(plan, none);
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()) == "a batch holds 1 to 8 assignments");
  }
  try {
    std::vector<std::vector<RingElem>> nine(9, x[0]);
    is_satisfied_batch(cs, nine);
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()) == "a batch holds 1 to 8 assignments");
  }
  try {
    std::vector<std::vector<RingElem>> full(x);
    full[2].pop_back();
    solve_batch(plan, full);
    EXPECT(false);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::string(e.what()) == "assignment does not match the constraint system");
  }

  if (fails) {
    std::fprintf(stderr, "r1cs_batch_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("r1cs_batch_run: OK digests %016llx %016llx %016llx\n", (unsigned long long)digest_of(solved[0]),
              (unsigned long long)digest_of(solved[1]), (unsigned long long)digest_of(solved[2]));
  return 0;
}
