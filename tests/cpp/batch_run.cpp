// batch_run.cpp -- run-time check of ringsnark::amd::groth16::prove_batch / rinocchio::prove_batch
// (include/ringsnark_amd/batch.hpp, batch.h) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: batch_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The six-constraint chain of keygen_run.cpp, three different statements.  prove_batch of the three on a generated key and
// on a seeded key, per scheme: every proof equals prover(pk, ...) of that member word for word, is accepted by verifier
// with the member's primary input and rejected with another member's.
#include <cstdio>
#include <cstdlib>
#include <random>

#include <ringsnark_amd/batch.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

static bool same(const EncodingElem &a, const EncodingElem &b) {
  if (a.is_empty() || b.is_empty()) return a.is_empty() == b.is_empty();
  return a.words() == b.words();
}
static bool same(const groth16::proof &a, const groth16::proof &b) { return same(a.A, b.A) && same(a.B, b.B) && same(a.C, b.C); }
static bool same(const rinocchio::proof &a, const rinocchio::proof &b) {
  return same(a.A, b.A) && same(a.A_prime, b.A_prime) && same(a.B, b.B) && same(a.B_prime, b.B_prime) && same(a.C, b.C) &&
         same(a.C_prime, b.C_prime) && same(a.D, b.D) && same(a.D_prime, b.D_prime) && same(a.F, b.F);
}

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

  const size_t m = 6, n_inputs = 2, n_vars = m + 2, B = 3;
  R1csCsr csr;
  csr.m = m;
  csr.n_vars = n_vars;
  csr.n_inputs = n_inputs;
  for (int w = 0; w < 3; w++) {
    csr.row_ptr[w].push_back(0);
    for (size_t i = 0; i < m; i++) {
      csr.col[w].push_back((uint32_t)(i + 1 + w));  // a: x_i, b: x_{i+1}, c: x_{i+2}; index 0 is the constant one
      csr.row_ptr[w].push_back((uint32_t)(i + 1));
    }
    csr.coeff[w].assign((size_t)p.L * m, 1);  // [L][nnz]
  }

  std::mt19937_64 g(11);
  auto random_unit = [&]() {
    std::vector<uint64_t> w(Context::ring_words());
    for (int i = 0; i < p.L; i++)
      for (int s = 0; s < p.N; s++) w[(size_t)i * p.N + s] = 1 + g() % (p.q[i] - 1);
    return RingElem(std::move(w));
  };
  std::vector<batch_input> inputs;
  for (size_t b = 0; b < B; b++) {
    std::vector<RingElem> x = {random_unit(), random_unit()};
    for (size_t i = 0; i < m; i++) x.push_back(x[i] * x[i + 1]);
    inputs.push_back(batch_input{std::vector<RingElem>(x.begin(), x.begin() + n_inputs), std::vector<RingElem>(x.begin() + n_inputs, x.end())});
  }

  {  // ringGroth16: a generated (full) key and a seeded one
    const auto full = groth16::generator(csr);
    const groth16::seeded_keypair half = groth16::generator(csr, seeded);
    const std::vector<groth16::proof> pf = groth16::prove_batch(full.pk, inputs), ph = groth16::prove_batch(half.pk, inputs);
    EXPECT(pf.size() == B && ph.size() == B);
    for (size_t b = 0; b < B && b < pf.size() && b < ph.size(); b++) {
      EXPECT(same(pf[b], groth16::prover(full.pk, inputs[b].primary, inputs[b].auxiliary)));
      EXPECT(same(ph[b], groth16::prover(half.pk, inputs[b].primary, inputs[b].auxiliary)));
      EXPECT(!same(pf[b], pf[(b + 1) % B]));
      for (size_t o = 0; o < B; o++) {
        EXPECT(groth16::verifier(full.vk, inputs[o].primary, pf[b]) == (o == b));
        EXPECT(groth16::verifier(half.vk, inputs[o].primary, ph[b]) == (o == b));
      }
    }
    bool refused = false;
    try {
      groth16::prove_batch(full.pk, std::vector<batch_input>(RS_MAX_BATCH + 1, inputs[0]));
    } catch (const std::invalid_argument &) {
      refused = true;
    }
    EXPECT(refused);
  }

  {  // Rinocchio, without blinding elements (proofs that prover repeats) and with the ones prove_batch samples
    const auto full = rinocchio::generator(csr);
    const rinocchio::seeded_keypair half = rinocchio::generator(csr, seeded);
    const std::vector<rinocchio::proof> pf = rinocchio::prove_batch(full.pk, inputs, nullptr), ph = rinocchio::prove_batch(half.pk, inputs, nullptr);
    const std::vector<rinocchio::proof> zf = rinocchio::prove_batch(full.pk, inputs), zh = rinocchio::prove_batch(half.pk, inputs);
    EXPECT(pf.size() == B && ph.size() == B && zf.size() == B && zh.size() == B);
    for (size_t b = 0; b < B && b < pf.size() && b < ph.size() && b < zf.size() && b < zh.size(); b++) {
      EXPECT(same(pf[b], rinocchio::prover(full.pk, inputs[b].primary, inputs[b].auxiliary, nullptr, nullptr, nullptr)));
      EXPECT(same(ph[b], rinocchio::prover(half.pk, inputs[b].primary, inputs[b].auxiliary, nullptr, nullptr, nullptr)));
      EXPECT(!same(zf[b], pf[b]));
      for (size_t o = 0; o < B; o++) {
        EXPECT(rinocchio::verifier(full.vk, inputs[o].primary, pf[b]) == (o == b));
        EXPECT(rinocchio::verifier(half.vk, inputs[o].primary, ph[b]) == (o == b));
        EXPECT(rinocchio::verifier(full.vk, inputs[o].primary, zf[b]) == (o == b));
        EXPECT(rinocchio::verifier(half.vk, inputs[o].primary, zh[b]) == (o == b));
      }
    }
    // explicit blinding elements: the batch equals prover with the same elements
    std::vector<rinocchio::blinding> d;
    for (size_t b = 0; b < B; b++) d.push_back(rinocchio::blinding{random_unit(), random_unit(), random_unit()});
    const std::vector<rinocchio::proof> df = rinocchio::prove_batch(full.pk, inputs, &d);
    for (size_t b = 0; b < B && b < df.size(); b++)
      EXPECT(same(df[b], rinocchio::prover(full.pk, inputs[b].primary, inputs[b].auxiliary, &d[b][0], &d[b][1], &d[b][2])));
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
    std::fprintf(stderr, "batch_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("batch_run: OK\n");
  return 0;
}
