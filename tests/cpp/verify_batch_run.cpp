// verify_batch_run.cpp -- run-time check of ringsnark::amd::groth16::verify_batch and ringsnark::amd::rinocchio::verify_batch
// (include/ringsnark_amd/verify_batch.hpp) against librs_hip.so: plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: verify_batch_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The six-constraint chain and the keys of verify_run.cpp.  Three assignments are proved per scheme; the batch holds their
// three proofs and a fourth member -- the second proof with a changed primary input.  Every verdict must be the single
// verifier's, report included; the same batch switched to K - 1 primes must give the same reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include <ringsnark_amd/verify_batch.hpp>

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
  return a.accepted == b.accepted && a.failed == b.failed && std::memcmp(a.n_bad, b.n_bad, sizeof(a.n_bad)) == 0 &&
         a.first_check == b.first_check && a.first_limb == b.first_limb && a.first_slot == b.first_slot && a.lhs == b.lhs && a.rhs == b.rhs;
}

static void print_verdicts(const char *scheme, const std::vector<batch_verdict> &v) {
  for (size_t b = 0; b < v.size(); b++)
    std::printf("%s member %zu: %s (budget %d, failed %u, first %u/%u/%u)\n", scheme, b,
                v[b].noise_spent ? "noise budget spent" : (v[b].accepted() ? "accepted" : "rejected"), v[b].budget_min, v[b].report.failed,
                v[b].report.first_check, v[b].report.first_limb, v[b].report.first_slot);
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
  auto random_unit = [&](uint64_t lo) {
    std::vector<uint64_t> w(Context::ring_words());
    for (int i = 0; i < p.L; i++)
      for (int s = 0; s < p.N; s++) w[(size_t)i * p.N + s] = lo + g() % (p.q[i] - lo);
    return RingElem(std::move(w));
  };
  // three assignments: primary inputs and auxiliary wires of each
  std::vector<std::vector<RingElem>> primaries, auxes;
  for (int t = 0; t < 3; t++) {
    std::vector<RingElem> x = {random_unit(1), random_unit(1)};
    for (size_t i = 0; i < m; i++) x.push_back(x[i] * x[i + 1]);
    primaries.emplace_back(x.begin(), x.begin() + n_inputs);
    auxes.emplace_back(x.begin() + n_inputs, x.end());
  }
  // the batch: the three proofs, then the second proof again with one slot of its second input changed
  std::vector<std::vector<RingElem>> batch_inputs = primaries;
  {
    std::vector<RingElem> bad = primaries[1];
    std::vector<uint64_t> w = bad[1].get_poly();
    const size_t at = (size_t)(p.L - 1) * p.N + 3;
    w[at] = (w[at] + 1) % p.q[p.L - 1];
    bad[1] = RingElem(std::move(w));
    batch_inputs.push_back(bad);
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
  const int K = p.K;

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
    std::vector<groth16::proof> proofs;
    for (int t = 0; t < 3; t++) proofs.push_back(groth16::prover(pk, primaries[t], auxes[t]));
    proofs.push_back(proofs[1]);
    const groth16::verification_key_device dvk(groth16::verification_key{csr, s, alpha, beta, gamma, delta, sk});
    const std::vector<batch_verdict> v = groth16::verify_batch(dvk, batch_inputs, proofs);
    print_verdicts("groth16", v);
    EXPECT(v.size() == 4 && v[0].accepted() && v[1].accepted() && v[2].accepted() && !v[3].accepted());
    EXPECT(v[3].report.failed == 1 && v[3].report.n_bad[0] == 1 && v[3].report.first_limb == (uint32_t)(p.L - 1) && v[3].report.first_slot == 3);
    for (size_t b = 0; b < v.size(); b++) {
      rs_verify_report rep;
      EXPECT(groth16::verifier(dvk, batch_inputs[b], proofs[b], &rep) == v[b].accepted());
      EXPECT(!v[b].noise_spent && v[b].budget_min > 0 && same_report(rep, v[b].report));
    }
    if (K > 1) {  // the same members switched to K - 1 primes
      std::vector<groth16::switched_proof> sw;
      for (const auto &pr : proofs) sw.push_back(groth16::mod_switch(pr, K - 1));
      const std::vector<batch_verdict> vs = groth16::verify_batch(dvk, batch_inputs, sw, K - 1);
      for (size_t b = 0; b < vs.size(); b++) EXPECT(!vs[b].noise_spent && same_report(vs[b].report, v[b].report));
    }
    try {
      groth16::verify_batch(dvk, primaries, proofs);  // three inputs, four proofs
      EXPECT(false);
    } catch (const std::invalid_argument &e) {
      EXPECT(std::string(e.what()) == "as many primary inputs as proofs");
    }
    EXPECT(groth16::verify_batch(dvk, {}, {}).empty());
    // more members than one call takes: successive calls, the same verdicts in order
    std::vector<std::vector<RingElem>> many_inputs;
    std::vector<groth16::proof> many;
    for (int b = 0; b < RS_VERIFY_BATCH_MAX + 3; b++) many_inputs.push_back(batch_inputs[b % 4]), many.push_back(proofs[b % 4]);
    const std::vector<batch_verdict> vm = groth16::verify_batch(dvk, many_inputs, many);
    EXPECT(vm.size() == many.size());
    for (size_t b = 0; b < vm.size(); b++) EXPECT(same_report(vm[b].report, v[b % 4].report));
  }

  {  // Rinocchio, without blinding elements
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
    std::vector<rinocchio::proof> proofs;
    for (int t = 0; t < 3; t++) proofs.push_back(rinocchio::prover(pk, primaries[t], auxes[t], nullptr, nullptr, nullptr));
    proofs.push_back(proofs[1]);
    std::swap(proofs[2].A_prime, proofs[2].B_prime);  // the third member tampered too: V' and W' exchanged
    proofs[0].F = EncodingElem();                      // the first without its last element: the L_beta check is skipped for it alone
    const rinocchio::verification_key_device dvk(rinocchio::verification_key{csr, s, alpha, beta, r_v, r_w, r_y, sk});
    const std::vector<batch_verdict> v = rinocchio::verify_batch(dvk, batch_inputs, proofs);
    print_verdicts("rinocchio", v);
    EXPECT(v.size() == 4 && v[0].accepted() && v[1].accepted() && !v[2].accepted() && !v[3].accepted());
    EXPECT(v[2].report.failed == 3u && v[3].report.failed == (1u << 5) && v[3].report.n_bad[5] == 1);
    for (size_t b = 0; b < v.size(); b++) {
      rs_verify_report rep;
      EXPECT(rinocchio::verifier(dvk, batch_inputs[b], proofs[b], &rep) == v[b].accepted());
      EXPECT(!v[b].noise_spent && v[b].budget_min > 0 && same_report(rep, v[b].report));
    }
  }

  if (fails) {
    std::fprintf(stderr, "verify_batch_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("verify_batch_run: OK\n");
  return 0;
}
