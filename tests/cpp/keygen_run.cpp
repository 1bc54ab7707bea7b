// keygen_run.cpp -- run-time check of ringsnark::amd::groth16::generator and ringsnark::amd::rinocchio::generator
// (include/ringsnark_amd/keygen.hpp) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: keygen_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// A six-constraint chain x_i * x_{i+1} = x_{i+2} (x_0, x_1 primary).  generator(cs) -> prover -> verifier accepts, rejects
// after a primary input is changed, and two generator calls give different trapdoors.
#include <cstdio>
#include <cstdlib>
#include <random>

#include <ringsnark_amd/keygen.hpp>

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

  const size_t m = 6, n_inputs = 2, n_vars = m + 2;
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
  std::vector<RingElem> x = {random_unit(), random_unit()};
  for (size_t i = 0; i < m; i++) x.push_back(x[i] * x[i + 1]);
  const std::vector<RingElem> primary(x.begin(), x.begin() + n_inputs), aux(x.begin() + n_inputs, x.end());
  std::vector<RingElem> bad_primary(primary);
  {
    std::vector<uint64_t> w = primary[1].get_poly();
    const size_t at = (size_t)(p.L - 1) * p.N + 3;
    w[at] = (w[at] + 1) % p.q[p.L - 1];
    bad_primary[1] = RingElem(std::move(w));
  }

  {  // ringGroth16
    const groth16::keypair kp = groth16::generator(csr);
    const groth16::proof proof = groth16::prover(kp.pk, primary, aux);
    EXPECT(!proof.A.is_empty() && !proof.B.is_empty() && !proof.C.is_empty());
    EXPECT(groth16::verifier(kp.vk, primary, proof));
    rs_verify_report rep;
    const groth16::verification_key_device dvk(kp.vk);
    EXPECT(!groth16::verifier(dvk, bad_primary, proof, &rep));
    EXPECT(rep.failed == 1 && rep.n_bad[0] == 1 && rep.first_limb == (uint32_t)(p.L - 1) && rep.first_slot == 3);
    const groth16::keypair again = groth16::generator(csr);
    EXPECT(again.vk.s.to_poly().get_poly() != kp.vk.s.to_poly().get_poly());
    EXPECT(again.vk.delta.get_poly() != kp.vk.delta.get_poly());
    EXPECT(again.vk.sk_enc != kp.vk.sk_enc);
    // a proof under one key is no proof under the other: rejected, or refused by the noise guard (the other secret key
    // decrypts it to noise, and the reference's decode throws there, seal_ring.tcc:446-454)
    try {
      EXPECT(!groth16::verifier(again.vk, primary, proof));
    } catch (const decoding_error &) {
    }
    EXPECT(groth16::verifier(again.vk, primary, groth16::prover(again.pk, primary, aux)));
  }

  {  // Rinocchio, without blinding elements and with the ones the prover samples
    const rinocchio::keypair kp = rinocchio::generator(csr);
    const rinocchio::proof proof = rinocchio::prover(kp.pk, primary, aux, nullptr, nullptr, nullptr);
    EXPECT(rinocchio::verifier(kp.vk, primary, proof));
    rs_verify_report rep;
    const rinocchio::verification_key_device dvk(kp.vk);
    EXPECT(!rinocchio::verifier(dvk, bad_primary, proof, &rep));
    EXPECT(rep.failed == (1u << 5) && rep.n_bad[5] == 1 && rep.first_limb == (uint32_t)(p.L - 1) && rep.first_slot == 3);
    EXPECT(rinocchio::verifier(dvk, primary, rinocchio::prover(kp.pk, primary, aux)));
    const rinocchio::keypair again = rinocchio::generator(csr);
    EXPECT(again.vk.s.to_poly().get_poly() != kp.vk.s.to_poly().get_poly());
    EXPECT(again.vk.r_y.get_poly() != kp.vk.r_y.get_poly());
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
    std::fprintf(stderr, "keygen_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("keygen_run: OK\n");
  return 0;
}
