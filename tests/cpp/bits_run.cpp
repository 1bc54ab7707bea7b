// bits_run.cpp -- run-time check of ringsnark::amd::bit_decompose (include/ringsnark_amd/bits.hpp) against librs_hip.so:
// plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: bits_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The range check by bit decomposition without constants (variable 1 the public wire `one`, then per block b_0 .. b_{logT-1}, x:
// b_i * (one - b_i) = 0, x * one = sum 2^i b_i), two blocks of logT = 8, written as R1csCsr by hand.  `one` and the x rows are
// uploaded, the bit rows are made on the device inside the assignment, is_satisfied holds, and the Rinocchio generator,
// prover and verifier accept.  An x with 2^logT in one slot is reported, and the assignment made from it is not satisfied.
#include <cstdio>
#include <cstdlib>
#include <random>

#include <ringsnark_amd/bits.hpp>
#include <ringsnark_amd/keygen.hpp>
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

static void run(int argc, char **argv) {
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

  const int logT = 8;
  const size_t count = 2, w = logT + 1, m = count * w, n_vars = 1 + count * w, rw = Context::ring_words();
  R1csCsr csr;
  csr.m = m;
  csr.n_vars = n_vars;
  csr.n_inputs = 1;
  std::vector<uint64_t> cf[3];  // one coefficient per non-zero, reduced per limb below
  for (int k = 0; k < 3; k++) csr.row_ptr[k].push_back(0);
  auto term = [&](int k, size_t var, uint64_t c) {
    csr.col[k].push_back((uint32_t)var);
    cf[k].push_back(c);
  };
  auto end_row = [&]() {
    for (int k = 0; k < 3; k++) csr.row_ptr[k].push_back((uint32_t)csr.col[k].size());
  };
  const uint64_t MINUS_ONE = ~0ull;  // marks the coefficient -1
  for (size_t blk = 0; blk < count; blk++) {
    const size_t b0 = 2 + blk * w, x = b0 + logT;  // 1-based variables; index 0 is the constant one, which no row uses
    for (int i = 0; i < logT; i++) {
      term(0, b0 + i, 1);
      term(1, 1, 1);
      term(1, b0 + i, MINUS_ONE);
      end_row();
    }
    term(0, x, 1);
    term(1, 1, 1);
    for (int i = 0; i < logT; i++) term(2, b0 + i, (uint64_t)1 << i);
    end_row();
  }
  for (int k = 0; k < 3; k++)
    for (int l = 0; l < p.L; l++)
      for (uint64_t c : cf[k]) csr.coeff[k].push_back(c == MINUS_ONE ? p.q[l] - 1 : c % p.q[l]);  // [L][nnz]
  const DeviceR1cs cs(csr);

  // one integer below 2^logT per slot, the same word in every limb
  std::mt19937_64 g(5);
  std::vector<uint64_t> h(n_vars * rw, 0xDEADull);
  for (size_t i = 0; i < rw; i++) h[i] = 1;
  for (size_t blk = 0; blk < count; blk++)
    for (int s = 0; s < p.N; s++) {
      const uint64_t v = s == 0 ? 0 : s == 1 ? ((uint64_t)1 << logT) - 1 : g() % ((uint64_t)1 << logT);
      for (int l = 0; l < p.L; l++) h[(1 + blk * w + logT) * rw + (size_t)l * p.N + s] = v;
    }
  DeviceWords asg(h.data(), h.size());
  rs_bits_report rep;
  EXPECT(bit_decompose(asg, 1 + logT, w, count, logT, asg, 1, w, &rep));
  EXPECT(rep.n_bad == 0 && rep.first_elem == 0 && rep.first_limb == 0 && rep.first_slot == 0 && rep.word == 0 && rep.value == 0);
  std::vector<uint64_t> full(h.size());
  asg.download(full.data());
  for (size_t blk = 0; blk < count; blk++)
    for (size_t i = 0; i < rw; i++) {
      const size_t xr = 1 + blk * w + logT;
      EXPECT(full[xr * rw + i] == h[xr * rw + i]);  // the x rows are as they were
      for (int k = 0; k < logT; k++) EXPECT(full[(1 + blk * w + k) * rw + i] == ((h[xr * rw + i % p.N] >> k) & 1));
    }
  for (size_t i = 0; i < rw; i++) EXPECT(full[i] == 1);

  std::vector<RingElem> wires;
  for (size_t v = 0; v < n_vars; v++) wires.emplace_back(std::vector<uint64_t>(full.begin() + v * rw, full.begin() + (v + 1) * rw));
  const std::vector<RingElem> primary(wires.begin(), wires.begin() + 1), aux(wires.begin() + 1, wires.end());
  EXPECT(is_satisfied(cs, primary, aux));

  // the single-element form gives the same rows
  const std::vector<RingElem> bits = bit_decompose(wires[1 + logT], logT, &rep);
  EXPECT(rep.n_bad == 0 && bits.size() == (size_t)logT);
  for (int k = 0; k < logT && k < (int)bits.size(); k++) EXPECT(bits[k].get_poly() == wires[1 + k].get_poly());

  {  // Rinocchio: generator -> prover -> verifier
    const rinocchio::keypair kp = rinocchio::generator(csr);
    const rinocchio::proof proof = rinocchio::prover(kp.pk, primary, aux, nullptr, nullptr, nullptr);
    EXPECT(rinocchio::verifier(kp.vk, primary, proof));
    EXPECT(rinocchio::verifier(kp.vk, primary, rinocchio::prover(kp.pk, primary, aux)));
  }

  {  // 2^logT in slot 3 of block 1: reported, and the packing constraint of that block fails at limb 0, slot 3
    const size_t xr = 1 + 1 * w + logT;
    std::vector<uint64_t> bad(h);
    for (int l = 0; l < p.L; l++) bad[xr * rw + (size_t)l * p.N + 3] = (uint64_t)1 << logT;
    DeviceWords dbad(bad.data(), bad.size());
    EXPECT(!bit_decompose(dbad, 1 + logT, w, count, logT, dbad, 1, w, &rep));
    EXPECT(rep.n_bad == 1 && rep.first_elem == 1 && rep.first_limb == 0 && rep.first_slot == 3);
    EXPECT(rep.word == ((uint64_t)1 << logT) && rep.value == ((uint64_t)1 << logT));
    dbad.download(bad.data());
    std::vector<RingElem> bw;
    for (size_t v = 0; v < n_vars; v++) bw.emplace_back(std::vector<uint64_t>(bad.begin() + v * rw, bad.begin() + (v + 1) * rw));
    r1cs_violation where{};
    EXPECT(!is_satisfied(cs, std::vector<RingElem>(bw.begin(), bw.begin() + 1), std::vector<RingElem>(bw.begin() + 1, bw.end()), &where));
    EXPECT(where.n_violated == 1 && where.constraint == 2 * w - 1 && where.limb == 0 && where.slot == 3);
  }

  try {  // an x row that is a bit row
    bit_decompose(asg, 1, w, count, logT, asg, 1, w, &rep);
    EXPECT(false);
  } catch (const std::exception &) {
  }
}

int main(int argc, char **argv) {
  try {
    run(argc, argv);
  } catch (const std::exception &e) {  // reported as a failure, not as an abort
    std::fprintf(stderr, "FAIL exception: %s\n", e.what());
    fails++;
  }
  if (fails) {
    std::fprintf(stderr, "bits_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("bits_run: OK\n");
  return 0;
}
