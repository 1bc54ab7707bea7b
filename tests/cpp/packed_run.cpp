// packed_run.cpp -- run-time check of the PACKED keys of ringsnark::amd::groth16::generator / rinocchio::generator
// (include/ringsnark_amd/packed.hpp, packed.h) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: packed_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The six-constraint chain of keygen_run.cpp.  generator(cs, packed) -> prover -> verifier accepts and rejects a changed
// primary input; the packed key is rs_enc_packed_words words an element; the proofs -- single and in a batch -- are, word for
// word, the ones the seeded prover gives for the SEEDED key of the same seeds: the packed vectors unpacked by rs_enc_unpack_c0.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include <ringsnark_amd/packed.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

// the compact vector of a packed one: rs_enc_unpack_c0
static DeviceWords unpacked(const DeviceWords &v) {
  const size_t count = v.words() / packed_words();
  EXPECT(count * packed_words() == v.words());
  DeviceWords c0(count * Context::enc_words() / 2);
  check(rs_enc_unpack_c0(Context::get_context(), v.get(), count, c0.get(), nullptr));
  return c0;
}
static DeviceWords copy_of(const DeviceWords &v) {
  std::vector<uint64_t> w(v.words());
  v.download(w.data());
  return DeviceWords(w.data(), w.size());
}
static std::vector<uint64_t> proof_words(std::initializer_list<const EncodingElem *> es) {
  std::vector<uint64_t> w;
  for (const EncodingElem *e : es) {
    EXPECT(!e->is_empty());
    const std::vector<uint64_t> x = e->words();
    w.insert(w.end(), x.begin(), x.end());
  }
  return w;
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
  const size_t ew = Context::enc_words(), pw = packed_words();
  const int w = rs_enc_pack_bits(Context::get_context());
  EXPECT(w >= 2 && w <= 62 && pw == (size_t)p.L * p.K * 2 * (((size_t)p.N_enc * w + 127) / 128) && pw <= ew / 2);
  const std::vector<batch_input> two = {batch_input{primary, aux}, batch_input{primary, aux}};

  {  // ringGroth16
    const groth16::packed_keypair kp = groth16::generator(csr, packed);
    EXPECT(kp.pk.s_pows_.words() == (m + 1) * pw && kp.pk.delta_ts_.words() == (m + 1) * pw && kp.pk.delta_mid_.words() == m * pw);
    EXPECT(kp.pk.alpha_.words() == ew && kp.pk.beta_.words() == ew);
    EXPECT(groth16::generator(csr, seeded).pk.s_pows_.words() == (m + 1) * ew / 2);  // the other tag: the seeded key of seeded.hpp
    const groth16::proof proof = groth16::prover(kp.pk, primary, aux);
    EXPECT(groth16::verifier(kp.vk, primary, proof));
    EXPECT(!groth16::verifier(kp.vk, bad_primary, proof));
    const groth16::seeded_proving_key same(csr, unpacked(kp.pk.s_pows_), unpacked(kp.pk.delta_ts_), unpacked(kp.pk.delta_mid_),
                                           copy_of(kp.pk.alpha_), copy_of(kp.pk.beta_), kp.pk.pub_seeds);
    const groth16::proof expected = groth16::prover(same, primary, aux);
    const std::vector<uint64_t> got = proof_words({&proof.A, &proof.B, &proof.C});
    EXPECT(got == proof_words({&expected.A, &expected.B, &expected.C}));
    const std::vector<groth16::proof> batch = groth16::prove_batch(kp.pk, two);
    EXPECT(batch.size() == 2);
    for (const groth16::proof &b : batch) EXPECT(got == proof_words({&b.A, &b.B, &b.C}));
  }

  {  // Rinocchio, without blinding elements (a proof that can be repeated) and with the ones the prover samples
    const rinocchio::packed_keypair kp = rinocchio::generator(csr, packed);
    EXPECT(kp.pk.s_pows_.words() == (m + 1) * pw && kp.pk.alpha_s_pows_.words() == (m + 1) * pw && kp.pk.beta_prods_.words() == m * pw);
    const rinocchio::proof proof = rinocchio::prover(kp.pk, primary, aux, nullptr, nullptr, nullptr);
    EXPECT(rinocchio::verifier(kp.vk, primary, proof));
    EXPECT(!rinocchio::verifier(kp.vk, bad_primary, proof));
    EXPECT(rinocchio::verifier(kp.vk, primary, rinocchio::prover(kp.pk, primary, aux)));
    const rinocchio::seeded_proving_key same(csr, unpacked(kp.pk.s_pows_), unpacked(kp.pk.alpha_s_pows_), unpacked(kp.pk.beta_prods_),
                                             copy_of(kp.pk.beta_rv_ts_), copy_of(kp.pk.beta_rw_ts_), copy_of(kp.pk.beta_ry_ts_),
                                             kp.pk.pub_seeds);
    const rinocchio::proof expected = rinocchio::prover(same, primary, aux, nullptr, nullptr, nullptr);
    auto words9 = [](const rinocchio::proof &q) {
      return proof_words({&q.A, &q.A_prime, &q.B, &q.B_prime, &q.C, &q.C_prime, &q.D, &q.D_prime, &q.F});
    };
    const std::vector<uint64_t> got = words9(proof);
    EXPECT(got == words9(expected));
    const std::vector<rinocchio::proof> batch = rinocchio::prove_batch(kp.pk, two, nullptr);
    EXPECT(batch.size() == 2);
    for (const rinocchio::proof &b : batch) EXPECT(got == words9(b));
    for (const rinocchio::proof &b : rinocchio::prove_batch(kp.pk, two)) EXPECT(rinocchio::verifier(kp.vk, primary, b));
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
    std::fprintf(stderr, "packed_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("packed_run: OK\n");
  return 0;
}
