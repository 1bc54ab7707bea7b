// solve_hints_run.cpp -- run-time check of ringsnark::amd::hint_plan / solve_hinted (include/ringsnark_amd/solve_hints.hpp)
// against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: solve_hints_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The running maximum of x_0, x_1, x_2 on 8-bit differences (ringsnark_amd.r1cs.running_max_r1cs(q, 8, 2), written here as
// R1csCsr): variables (0-based) one 0, x_0..x_2 1..3, then per stage j: s_j, b_{j,0..7}, m_j from 4 + 10 j;
//   (m_{j-1} - x_{j+1} + 128 one) * one = s_j,  b (one - b) = 0 per bit,  s_j * one = sum 2^k b_{j,k},
//   b_{j,7} (m_{j-1} - x_{j+1}) = m_j - x_{j+1},          hint BITS(s_j -> b_j)
// with x_0[s] = (5 s + 3) % 128, x_1[s] = (11 s + 70) % 128, x_2[s] = (s s) % 128 in every limb; solved from {one, x} in every
// mode, accepted by is_satisfied, m_1 = max(x_0, x_1, x_2); then a division y = c / t with a zero planted in t.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include <ringsnark_amd/r1cs_check.hpp>
#include <ringsnark_amd/solve_hints.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

using Terms = std::vector<std::pair<uint32_t, int64_t>>;  // (column: 0 the constant one, variable v is v + 1; signed literal)

struct Builder {
  const Params &p;
  R1csCsr csr;
  std::vector<int64_t> lit[3];
  explicit Builder(const Params &prm) : p(prm) {
    for (int w = 0; w < 3; w++) csr.row_ptr[w].push_back(0);
  }
  void add(const Terms &a, const Terms &b, const Terms &c) {
    const Terms *rows[3] = {&a, &b, &c};
    for (int w = 0; w < 3; w++) {
      for (const auto &t : *rows[w]) {
        csr.col[w].push_back(t.first);
        lit[w].push_back(t.second);
      }
      csr.row_ptr[w].push_back((uint32_t)csr.col[w].size());
    }
    csr.m++;
  }
  R1csCsr finish(size_t n_vars, size_t n_inputs) {
    csr.n_vars = n_vars;
    csr.n_inputs = n_inputs;
    for (int w = 0; w < 3; w++)  // [L][nnz]: a literal c < 0 is the negation of -c modulo q_l
      for (int l = 0; l < p.L; l++)
        for (const int64_t c : lit[w]) csr.coeff[w].push_back(c < 0 ? p.q[l] - (uint64_t)(-c) % p.q[l] : (uint64_t)c % p.q[l]);
    return csr;
  }
};

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
  const size_t rw = Context::ring_words();

  // ---- the running maximum
  const uint32_t nbits = 8, count = 2, one = 1;
  Builder bm(p);
  std::vector<rs_solve_hint> hints;
  uint32_t prev = 2;  // columns from here on
  for (uint32_t j = 0; j < count; j++) {
    const uint32_t x = 3 + j, s = count + 3 + j * (nbits + 2), mx = s + 1 + nbits;
    bm.add({{prev, 1}, {x, -1}, {one, 128}}, {{one, 1}}, {{s, 1}});
    Terms pack;
    for (uint32_t k = 0; k < nbits; k++) {
      bm.add({{s + 1 + k, 1}}, {{one, 1}, {s + 1 + k, -1}}, {});
      pack.push_back({s + 1 + k, (int64_t)1 << k});
    }
    bm.add({{s, 1}}, {{one, 1}}, pack);
    bm.add({{s + nbits, 1}}, {{prev, 1}, {x, -1}}, {{mx, 1}, {x, -1}});
    hints.push_back(bits_hint(s - 1, s, nbits));
    prev = mx;
  }
  const size_t nv = count + 2 + count * (nbits + 2);
  const DeviceR1cs cs(bm.finish(nv, count + 2));
  std::vector<RingElem> x(nv);  // the unknown wires: default-constructed
  std::vector<uint64_t> xs[3];
  x[0] = RingElem(std::vector<uint64_t>(rw, 1));
  for (int k = 0; k < 3; k++) {
    xs[k].resize(rw);
    for (int l = 0; l < p.L; l++)
      for (uint64_t s = 0; s < (uint64_t)p.N; s++) xs[k][(size_t)l * p.N + s] = (k == 0 ? 5 * s + 3 : k == 1 ? 11 * s + 70 : s * s) % 128;
    x[1 + k] = RingElem(xs[k]);
  }
  std::vector<bool> given(nv, false);
  for (size_t v = 0; v < count + 2; v++) given[v] = true;
  const hint_plan plan(cs, given, hints);
  const rs_r1cs_hint_info &info = plan.info();
  EXPECT(info.solve.n_given == count + 2 && info.solve.n_solved == count * (nbits + 2) && info.solve.n_unsolved == 0);
  EXPECT(info.solve.n_levels == 3 * count && info.n_steps == 3 * count && info.solve.max_width == 1 && info.solve.blocked_reason == 0);
  EXPECT(info.n_hints_run == count && info.n_hints_blocked == 0 && info.first_blocked_hint == count);
  const std::vector<uint32_t> wires = plan.solved_wires();
  EXPECT(wires.size() == count * (nbits + 2));
  for (size_t i = 0; i < wires.size(); i++) EXPECT(wires[i] == count + 2 + i);

  uint64_t digest[3];
  for (int mode = 0; mode < 3; mode++) {
    std::vector<RingElem> full(x);
    rs_solve_hint_report rep;
    const rs_r1cs_hint_stats st = solve_hinted(plan, full, mode, &rep);
    if (mode == RS_SOLVE_LEVELS) EXPECT(st.level_launches == 2 * count && st.walk_launches == 0 && st.hint_launches == count);
    else EXPECT(st.level_launches == 0 && st.walk_launches == count + 1 && st.hint_launches == count);
    EXPECT(rep.n_bits_bad == 0 && rep.n_zero == 0);
    EXPECT(is_satisfied(cs, std::vector<RingElem>(full.begin(), full.begin() + count + 2), std::vector<RingElem>(full.begin() + count + 2, full.end())));
    const std::vector<uint64_t> &m1 = full[nv - 1].get_poly();
    for (size_t i = 0; i < rw; i++) EXPECT(m1[i] == std::max(xs[0][i], std::max(xs[1][i], xs[2][i])));
    uint64_t h = 0xcbf29ce484222325ull;
    for (const uint64_t v : flatten(full)) h = (h ^ v) * 0x100000001b3ull;
    digest[mode] = h;
  }
  EXPECT(digest[0] == digest[1] && digest[1] == digest[2]);

  // without the second hint: stage 1's bits and m_1 stay unsolved
  {
    const hint_plan partial(cs, given, std::vector<rs_solve_hint>(hints.begin(), hints.begin() + 1));
    EXPECT(partial.info().solve.n_unsolved == nbits + 1 && partial.info().solve.first_unsolved == nv - nbits - 1);
    try {
      std::vector<RingElem> full(x);
      solve_hinted(partial, full);
      EXPECT(false);
    } catch (const std::invalid_argument &e) {
      EXPECT(std::string(e.what()).find("first unsolved variable " + std::to_string(nv - nbits - 1) + ",") != std::string::npos);
    }
  }
  // a refused hint: its target is given
  try {
    const hint_plan refused(cs, given, {inv_hint(1, 2)});
    EXPECT(false);
  } catch (const std::exception &) {
  }

  // ---- t = y + d, z = c / t with the quotient hint; t is zero in slot 3 of the last limb, and so is c there
  Builder bd(p);
  bd.add({{2, 1}, {4, 1}}, {{1, 1}}, {{5, 1}});  // variables: one 0, y 1, c 2, d 3, t 4, z 5
  bd.add({{6, 1}}, {{5, 1}}, {{3, 1}});
  const DeviceR1cs ds(bd.finish(6, 4));
  std::vector<RingElem> w(6);
  w[0] = RingElem(std::vector<uint64_t>(rw, 1));
  std::vector<uint64_t> y(rw), c(rw), d(rw);
  for (int l = 0; l < p.L; l++)
    for (uint64_t s = 0; s < (uint64_t)p.N; s++) {
      const size_t i = (size_t)l * p.N + s;
      y[i] = (3 * s + 1 + l) % p.q[l];
      c[i] = (s * s + 7) % p.q[l];
      d[i] = (2 * s + 5) % p.q[l];
    }
  const size_t zi = (size_t)(p.L - 1) * p.N + 3;
  d[zi] = p.q[p.L - 1] - y[zi];
  c[zi] = 0;
  w[1] = RingElem(y), w[2] = RingElem(c), w[3] = RingElem(d);
  const hint_plan dplan(ds, {true, true, true, true, false, false}, {quot_hint(2, 4, 5)});
  EXPECT(dplan.info().solve.n_unsolved == 0 && dplan.info().solve.n_levels == 2);
  for (int mode = 0; mode < 3; mode++) {
    std::vector<RingElem> full(w);
    rs_solve_hint_report rep;
    const rs_r1cs_hint_stats st = solve_hinted(dplan, full, mode, &rep);
    EXPECT(st.hint_launches == (mode == RS_SOLVE_LEVELS ? 1u : 0u));
    EXPECT(rep.n_zero == 1 && rep.zero_hint == 0 && rep.zero_limb == (uint32_t)(p.L - 1) && rep.zero_slot == 3 && rep.n_bits_bad == 0);
    EXPECT(is_satisfied(ds, std::vector<RingElem>(full.begin(), full.begin() + 4), std::vector<RingElem>(full.begin() + 4, full.end())));
    EXPECT(full[5].get_poly()[zi] == 0);
    EXPECT((full[5] * full[4]).to_poly().get_poly() == c);
  }

  if (fails) {
    std::fprintf(stderr, "solve_hints_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("solve_hints_run: OK digest %016llx\n", (unsigned long long)digest[0]);
  return 0;
}
