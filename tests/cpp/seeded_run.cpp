// seeded_run.cpp -- run-time check of the SEEDED keys of ringsnark::amd::groth16::generator / rinocchio::generator
// (include/ringsnark_amd/seeded.hpp, seeded.h) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: seeded_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1} OUTDIR
// The six-constraint chain of keygen_run.cpp.  generator(cs, seeded) -> prover -> verifier accepts and rejects a changed
// primary input; the seeded key is half the size of the full one.  The compact key, its public seeds, the assignment and the
// proofs are written to OUTDIR as raw uint64 words, for tests/test_seeded_cpp.py to prove with the same key from Python.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include <ringsnark_amd/seeded.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

static std::string outdir;
static void dump(const char *name, const uint64_t *w, size_t n) {
  const std::string path = outdir + "/" + name;
  FILE *f = std::fopen(path.c_str(), "wb");
  EXPECT(f != nullptr);
  if (!f) return;
  EXPECT(std::fwrite(w, sizeof(uint64_t), n, f) == n);
  std::fclose(f);
}
static void dump(const char *name, const DeviceWords &d) {
  std::vector<uint64_t> w(d.words());
  if (d.words()) d.download(w.data());
  dump(name, w.data(), w.size());
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
  EXPECT(a + 1 == argc);
  outdir = argv[a];
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
  const std::vector<uint64_t> asg = flatten(x);
  dump("assignment.bin", asg.data(), asg.size());
  const size_t ew = Context::enc_words();

  {  // ringGroth16
    const groth16::seeded_keypair kp = groth16::generator(csr, seeded);
    EXPECT(kp.pk.s_pows_.words() == (m + 1) * ew / 2 && kp.pk.delta_ts_.words() == (m + 1) * ew / 2 && kp.pk.delta_mid_.words() == m * ew / 2);
    EXPECT(kp.pk.alpha_.words() == ew && kp.pk.beta_.words() == ew);
    EXPECT(groth16::generator(csr).pk.s_pows_.words() == (m + 1) * ew);  // without the tag: the full key of keygen.hpp
    const groth16::proof proof = groth16::prover(kp.pk, primary, aux);
    EXPECT(groth16::verifier(kp.vk, primary, proof));
    EXPECT(!groth16::verifier(kp.vk, bad_primary, proof));
    const groth16::seeded_keypair again = groth16::generator(csr, seeded);
    EXPECT(again.pk.pub_seeds[0] != kp.pk.pub_seeds[0]);
    dump("g_s_pows.bin", kp.pk.s_pows_);
    dump("g_delta_ts.bin", kp.pk.delta_ts_);
    dump("g_delta_mid.bin", kp.pk.delta_mid_);
    dump("g_alpha.bin", kp.pk.alpha_);
    dump("g_beta.bin", kp.pk.beta_);
    dump("g_pub.bin", kp.pk.pub_seeds, 5);
    const std::vector<uint64_t> w = proof_words({&proof.A, &proof.B, &proof.C});
    dump("g_proof.bin", w.data(), w.size());
  }

  {  // Rinocchio, without blinding elements (a proof Python can repeat) and with the ones the prover samples
    const rinocchio::seeded_keypair kp = rinocchio::generator(csr, seeded);
    EXPECT(kp.pk.s_pows_.words() == (m + 1) * ew / 2 && kp.pk.beta_prods_.words() == m * ew / 2);
    const rinocchio::proof proof = rinocchio::prover(kp.pk, primary, aux, nullptr, nullptr, nullptr);
    EXPECT(rinocchio::verifier(kp.vk, primary, proof));
    EXPECT(!rinocchio::verifier(kp.vk, bad_primary, proof));
    EXPECT(rinocchio::verifier(kp.vk, primary, rinocchio::prover(kp.pk, primary, aux)));
    dump("r_s_pows.bin", kp.pk.s_pows_);
    dump("r_alpha_s_pows.bin", kp.pk.alpha_s_pows_);
    dump("r_beta_prods.bin", kp.pk.beta_prods_);
    dump("r_beta_rv_ts.bin", kp.pk.beta_rv_ts_);
    dump("r_beta_rw_ts.bin", kp.pk.beta_rw_ts_);
    dump("r_beta_ry_ts.bin", kp.pk.beta_ry_ts_);
    dump("r_pub.bin", kp.pk.pub_seeds, 6);
    const std::vector<uint64_t> w = proof_words({&proof.A, &proof.A_prime, &proof.B, &proof.B_prime, &proof.C, &proof.C_prime, &proof.D,
                                                 &proof.D_prime, &proof.F});
    dump("r_proof.bin", w.data(), w.size());
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
    std::fprintf(stderr, "seeded_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("seeded_run: OK\n");
  return 0;
}
