// modswitch_run.cpp -- run-time check of ringsnark::amd::mod_switch and the verifier overloads on switched proofs
// (include/ringsnark_amd/modswitch.hpp) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: modswitch_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}      (K >= 2)
// The six-constraint chain of verify_run.cpp, keys generated the way the reference's generators do.  Each scheme's proof is
// switched to K - 1 primes; the verifier accepts it, rejects it for a changed primary input with the report of the
// unswitched proof, and a switched element decodes to what the unswitched one decodes to.
#include <cstdio>
#include <cstdlib>
#include <random>

#include <ringsnark_amd/modswitch.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

static std::vector<RingElem> rows_of(const DeviceWords &d, size_t rows) {
  const size_t rw = Context::ring_words();
  std::vector<uint64_t> w(rows * rw);
  d.download(w.data());
  std::vector<RingElem> out;
  for (size_t k = 0; k < rows; k++) out.emplace_back(std::vector<uint64_t>(w.begin() + k * rw, w.begin() + (k + 1) * rw));
  return out;
}

static bool same_report(const rs_verify_report &a, const rs_verify_report &b) {
  bool same = a.accepted == b.accepted && a.failed == b.failed && a.first_check == b.first_check && a.first_limb == b.first_limb &&
              a.first_slot == b.first_slot && a.lhs == b.lhs && a.rhs == b.rhs;
  for (int c = 0; c < 6; c++) same = same && a.n_bad[c] == b.n_bad[c];
  return same;
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
  EXPECT(a == argc && p.K >= 2);
  Context::set_context(p);
  const int lvl = p.K - 1;

  const size_t m = 6, n_inputs = 2, n_vars = m + 2, n_aux = n_vars - n_inputs;
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

  std::mt19937_64 g(13);
  auto random_unit = [&](uint64_t lo) {  // residues in [lo, q_i): non-zero, and for lo = m off every node of the domain
    std::vector<uint64_t> w(Context::ring_words());
    for (int i = 0; i < p.L; i++)
      for (int s = 0; s < p.N; s++) w[(size_t)i * p.N + s] = lo + g() % (p.q[i] - lo);
    return RingElem(std::move(w));
  };
  std::vector<RingElem> x = {random_unit(1), random_unit(1)};
  for (size_t i = 0; i < m; i++) x.push_back(x[i] * x[i + 1]);
  const std::vector<RingElem> primary(x.begin(), x.begin() + n_inputs), aux(x.begin() + n_inputs, x.end());
  std::vector<RingElem> bad_primary(primary);
  {
    std::vector<uint64_t> w = primary[1].get_poly();
    const size_t at = (size_t)(p.L - 1) * p.N + 3;
    w[at] = (w[at] + 1) % p.q[p.L - 1];
    bad_primary[1] = RingElem(std::move(w));
  }

  const RingElem s = random_unit(m);
  std::vector<RingElem> At, Bt, Ct, Ht;
  RingElem Zt;
  {
    const DeviceR1cs cs(csr);
    const size_t rw = Context::ring_words();
    const DeviceWords ds = upload_words(s.get_poly());
    DeviceWords dA((n_vars + 1) * rw), dB((n_vars + 1) * rw), dC((n_vars + 1) * rw), dH((m + 1) * rw), dZ(rw);
    check(rs_instance_map_eval(Context::get_context(), cs.get(), ds.get(), dA.get(), dB.get(), dC.get(), dH.get(), dZ.get(), nullptr));
    At = rows_of(dA, n_vars + 1), Bt = rows_of(dB, n_vars + 1), Ct = rows_of(dC, n_vars + 1), Ht = rows_of(dH, m + 1);
    Zt = rows_of(dZ, 1)[0];
  }
  const auto keys = EncodingElem::keygen();
  const EncodingElem::SecretKey &sk = std::get<1>(keys);

  {  // ringGroth16
    const RingElem alpha = random_unit(1), beta = random_unit(1), gamma = random_unit(1), delta = random_unit(1);
    const RingElem delta_inv = delta.inverse();
    std::vector<RingElem> delta_ts, delta_mid;
    for (size_t i = 0; i <= m; i++) delta_ts.push_back(Ht[i] * Zt * delta_inv);
    for (size_t i = 0; i < n_aux; i++) {
      const size_t idx = i + n_inputs + 1;
      delta_mid.push_back((beta * At[idx] + alpha * Bt[idx] + Ct[idx]) * delta_inv);
    }
    const groth16::proving_key_device pk(csr, EncodingElem::encode(sk, Ht, 1), EncodingElem::encode(sk, delta_ts, 2),
                                         EncodingElem::encode(sk, delta_mid, 3), EncodingElem::encode(sk, {alpha}, 4)[0],
                                         EncodingElem::encode(sk, {beta}, 5)[0]);
    const groth16::proof proof = groth16::prover(pk, primary, aux);
    const groth16::switched_proof sw = groth16::mod_switch(proof, lvl);
    EXPECT(sw.level == lvl && sw.A.level() == lvl && sw.A.words().size() == SwitchedEncodingElem::level_words(lvl));
    EXPECT(sw.size_in_bits() < proof.size_in_bits());
    EXPECT(SwitchedEncodingElem::decode(sk, sw.A) == EncodingElem::decode(sk, proof.A));
    EXPECT(SwitchedEncodingElem::decode(sk, mod_switch(proof.C, lvl)) == EncodingElem::decode(sk, proof.C));
    const groth16::verification_key vk{csr, s, alpha, beta, gamma, delta, sk};
    EXPECT(groth16::verifier(vk, primary, sw));  // the reference's signature, on the switched proof
    const groth16::verification_key_device dvk(vk);
    rs_verify_report rep, full;
    EXPECT(groth16::verifier(dvk, primary, sw, &rep) && groth16::verifier(dvk, primary, proof, &full) && same_report(rep, full));
    EXPECT(!groth16::verifier(dvk, bad_primary, sw, &rep) && !groth16::verifier(dvk, bad_primary, proof, &full));
    EXPECT(same_report(rep, full) && rep.failed == 1 && rep.n_bad[0] == 1 && rep.first_limb == (uint32_t)(p.L - 1) && rep.first_slot == 3);
    EXPECT(groth16::verifier(dvk, primary, groth16::mod_switch(proof, p.K)));  // level K: the proof itself
    try {
      groth16::mod_switch(proof, 0);
      EXPECT(false);
    } catch (const std::invalid_argument &e) {
      EXPECT(std::string(e.what()) == "level out of range");
    }
  }

  {  // Rinocchio, without blinding elements (d1 = d2 = d3 = 0)
    const RingElem alpha = random_unit(1), r_v = random_unit(1), r_w = random_unit(1), beta = random_unit(1);
    const RingElem r_y = r_v * r_w;
    std::vector<RingElem> alpha_s_pows, beta_prods;
    for (size_t i = 0; i <= m; i++) alpha_s_pows.push_back(Ht[i] * alpha);
    for (size_t i = 0; i < n_aux; i++) {
      const size_t idx = i + n_inputs + 1;
      beta_prods.push_back((r_v * At[idx] + r_w * Bt[idx] + r_y * Ct[idx]) * beta);
    }
    const RingElem beta_Zt = beta * Zt;
    const rinocchio::proving_key_device pk(csr, EncodingElem::encode(sk, Ht, 6), EncodingElem::encode(sk, alpha_s_pows, 7),
                                           EncodingElem::encode(sk, beta_prods, 8), EncodingElem::encode(sk, {beta_Zt * r_v}, 9)[0],
                                           EncodingElem::encode(sk, {beta_Zt * r_w}, 10)[0],
                                           EncodingElem::encode(sk, {beta_Zt * r_y}, 11)[0]);
    const rinocchio::proof proof = rinocchio::prover(pk, primary, aux, nullptr, nullptr, nullptr);
    const rinocchio::switched_proof sw = rinocchio::mod_switch(proof, lvl);
    const rinocchio::verification_key vk{csr, s, alpha, beta, r_v, r_w, r_y, sk};
    EXPECT(rinocchio::verifier(vk, primary, sw));
    const rinocchio::verification_key_device dvk(vk);
    rs_verify_report rep, full;
    EXPECT(rinocchio::verifier(dvk, primary, sw, &rep) && rep.accepted == 1 && rep.failed == 0);
    EXPECT(!rinocchio::verifier(dvk, bad_primary, sw, &rep) && !rinocchio::verifier(dvk, bad_primary, proof, &full));
    EXPECT(same_report(rep, full) && rep.failed == (1u << 5) && rep.n_bad[5] == 1 && rep.first_check == 5);
    rinocchio::proof no_aux = proof;  // an EMPTY last element stays EMPTY and skips the L_beta check
    no_aux.F = EncodingElem();
    const rinocchio::switched_proof sw_no_aux = rinocchio::mod_switch(no_aux, lvl);
    EXPECT(sw_no_aux.F.is_empty() && !sw_no_aux.D_prime.is_empty());
    EXPECT(rinocchio::verifier(dvk, primary, sw_no_aux, &rep));
  }

  if (fails) {
    std::fprintf(stderr, "modswitch_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("modswitch_run: OK\n");
  return 0;
}
