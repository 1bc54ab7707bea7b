// seeded.hpp -- header-only C++ adapter of seeded proving keys (seeded.h) on the types of ring.hpp, verify.hpp and keygen.hpp.
// A header of its own, beside keygen.hpp, for the reason given in r1cs_check.h: the adapters that exist stay as they are.
//
// generator(cs, seeded) -- the tag `ringsnark::amd::seeded` after the constraint system -- samples the trapdoor as
// generator(cs) of keygen.hpp does and returns {seeded_proving_key, verification_key}: the three vectors of the key keep
// their c0 halves only, half the device memory, and the key remembers the public seeds their c1 halves are regenerated from.
// The public seeds are drawn apart from the private ones (seeded.h "TWO SEEDS PER VECTOR"), from the same generator.
// prover(pk, ...) on a seeded_proving_key calls rs_groth16_prove_seeded / rs_rinocchio_prove_seeded.
#ifndef RINGSNARK_AMD_SEEDED_HPP
#define RINGSNARK_AMD_SEEDED_HPP

#include <algorithm>

#include "keygen.hpp"
#include "seeded.h"

namespace ringsnark::amd {

struct seeded_t {};
inline constexpr seeded_t seeded{};

namespace groth16 {
// s_pows_, delta_ts_, delta_mid_ are COMPACT [count][L][K][N_enc]; alpha_, beta_ full elements.  Only the prover below
// reads such a key: the provers of ring.hpp take the vectors for full-format ones.
struct seeded_proving_key : generated_proving_key {
  seeded_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords delta_ts, DeviceWords delta_mid, DeviceWords alpha,
                     DeviceWords beta, const uint64_t (&pub)[5])
      : generated_proving_key(cs_, std::move(s_pows), std::move(delta_ts), std::move(delta_mid), std::move(alpha), std::move(beta)) {
    std::copy(pub, pub + 5, pub_seeds);
  }
  uint64_t pub_seeds[5];  // of s_pows, delta_ts, delta_mid, alpha, beta
};
struct seeded_keypair {
  seeded_proving_key pk;
  verification_key vk;
};
// groth16::generator (groth16.tcc:5-66) with a seeded proving key
inline seeded_keypair generator(const R1csCsr &cs, seeded_t) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words(), kw = ew / 2;
  const RingElem s = detail::random_point(m);
  const EncodingElem::SecretKey sk = std::get<1>(EncodingElem::keygen());
  const RingElem alpha = RingElem::random_invertible_element(), beta = RingElem::random_invertible_element(),
                 gamma = RingElem::random_invertible_element(), delta = RingElem::random_invertible_element();
  uint64_t seeds[5], pub[5];
  detail::keygen_seeds(seeds);
  detail::keygen_seeds(pub);
  const DeviceR1cs dcs(cs);
  const DeviceWords ds = detail::upload_ring(s), dalpha = detail::upload_ring(alpha), dbeta = detail::upload_ring(beta),
                    ddelta = detail::upload_ring(delta), dsk = upload_words(sk);
  DeviceWords s_pows((m + 1) * kw), delta_ts((m + 1) * kw), delta_mid(n_aux * kw), ealpha(ew), ebeta(ew);
  rs_groth16_seeded_key_out out{};
  out.s_pows = s_pows.get(), out.delta_ts = delta_ts.get(), out.delta_mid = delta_mid.get();
  out.d_alpha = ealpha.get(), out.d_beta = ebeta.get();
  check(rs_groth16_keygen_seeded(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), ddelta.get(), dsk.get(), seeds,
                                 pub, &out, nullptr));
  return seeded_keypair{seeded_proving_key(cs, std::move(s_pows), std::move(delta_ts), std::move(delta_mid), std::move(ealpha),
                                           std::move(ebeta), pub),
                        verification_key{cs, s, alpha, beta, gamma, delta, sk}};
}
// groth16::prover (groth16.tcc:70-115) on a seeded key
inline proof prover(const seeded_proving_key &pk, const std::vector<RingElem> &primary_input,
                    const std::vector<RingElem> &auxiliary_input) {
  if (primary_input.size() != pk.cs.n_inputs || primary_input.size() + auxiliary_input.size() != pk.cs.n_vars)
    throw std::invalid_argument("assignment does not match the constraint system");
  std::vector<RingElem> full(primary_input);
  full.insert(full.end(), auxiliary_input.begin(), auxiliary_input.end());
  const std::vector<uint64_t> asg = flatten(full);
  DeviceWords dasg(asg.data(), asg.size()), dproof(3 * Context::enc_words());
  rs_groth16_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.delta_ts = pk.delta_ts_.get(), k.delta_mid = pk.delta_mid_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_alpha = pk.alpha_.get(), k.d_beta = pk.beta_.get();
  int empty[3] = {0, 0, 0};
  const std::vector<uint8_t> kinds = wire_kinds(full);
  check(rs_groth16_prove_seeded(Context::get_context(), pk.cs.get(), &k, dasg.get(), kinds.data(), dproof.get(), empty, nullptr));
  std::vector<uint64_t> w(3 * Context::enc_words());
  dproof.download(w.data());
  proof p;
  EncodingElem *dst[3] = {&p.A, &p.B, &p.C};
  for (int i = 0; i < 3; i++)
    if (!empty[i]) *dst[i] = take_element(w, i);
  return p;
}
}  // namespace groth16

namespace rinocchio {
// as groth16::seeded_proving_key: s_pows_, alpha_s_pows_, beta_prods_ compact
struct seeded_proving_key : generated_proving_key {
  seeded_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords alpha_s_pows, DeviceWords beta_prods, DeviceWords beta_rv_ts,
                     DeviceWords beta_rw_ts, DeviceWords beta_ry_ts, const uint64_t (&pub)[6])
      : generated_proving_key(cs_, std::move(s_pows), std::move(alpha_s_pows), std::move(beta_prods), std::move(beta_rv_ts),
                              std::move(beta_rw_ts), std::move(beta_ry_ts)) {
    std::copy(pub, pub + 6, pub_seeds);
  }
  uint64_t pub_seeds[6];  // of s_pows, alpha_s_pows, beta_prods, beta_rv_ts, beta_rw_ts, beta_ry_ts
};
struct seeded_keypair {
  seeded_proving_key pk;
  verification_key vk;
};
// rinocchio::generator (rinocchio.tcc:5-72) with a seeded proving key
inline seeded_keypair generator(const R1csCsr &cs, seeded_t) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words(), kw = ew / 2;
  const RingElem s = detail::random_point(m);
  const EncodingElem::SecretKey sk = std::get<1>(EncodingElem::keygen());
  const RingElem alpha = RingElem::random_invertible_element(), r_v = RingElem::random_invertible_element(),
                 r_w = RingElem::random_invertible_element(), r_y = r_v * r_w, beta = RingElem::random_nonzero_element();
  uint64_t seeds[6], pub[6];
  detail::keygen_seeds(seeds);
  detail::keygen_seeds(pub);
  const DeviceR1cs dcs(cs);
  const DeviceWords ds = detail::upload_ring(s), dalpha = detail::upload_ring(alpha), dbeta = detail::upload_ring(beta),
                    drv = detail::upload_ring(r_v), drw = detail::upload_ring(r_w), dry = detail::upload_ring(r_y), dsk = upload_words(sk);
  DeviceWords s_pows((m + 1) * kw), alpha_s_pows((m + 1) * kw), beta_prods(n_aux * kw), rv_ts(ew), rw_ts(ew), ry_ts(ew);
  rs_rinocchio_seeded_key_out out{};
  out.s_pows = s_pows.get(), out.alpha_s_pows = alpha_s_pows.get(), out.beta_prods = beta_prods.get();
  out.d_beta_rv_ts = rv_ts.get(), out.d_beta_rw_ts = rw_ts.get(), out.d_beta_ry_ts = ry_ts.get();
  check(rs_rinocchio_keygen_seeded(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), drv.get(), drw.get(), dry.get(),
                                   dsk.get(), seeds, pub, &out, nullptr));
  return seeded_keypair{seeded_proving_key(cs, std::move(s_pows), std::move(alpha_s_pows), std::move(beta_prods), std::move(rv_ts),
                                           std::move(rw_ts), std::move(ry_ts), pub),
                        verification_key{cs, s, alpha, beta, r_v, r_w, r_y, sk}};
}
// rinocchio::prover (rinocchio.tcc:75-190) on a seeded key; d1, d2, d3 as in ring.hpp
inline proof prover(const seeded_proving_key &pk, const std::vector<RingElem> &primary_input,
                    const std::vector<RingElem> &auxiliary_input, const RingElem *d1, const RingElem *d2, const RingElem *d3) {
  if (primary_input.size() != pk.cs.n_inputs || primary_input.size() + auxiliary_input.size() != pk.cs.n_vars)
    throw std::invalid_argument("assignment does not match the constraint system");
  std::vector<RingElem> full(primary_input);
  full.insert(full.end(), auxiliary_input.begin(), auxiliary_input.end());
  const std::vector<uint64_t> asg = flatten(full);
  DeviceWords dasg(asg.data(), asg.size()), dproof(9 * Context::enc_words());
  DeviceWords dd[3];
  const uint64_t *dp[3] = {nullptr, nullptr, nullptr};
  if (d1) {
    const RingElem *ds[3] = {d1, d2, d3};
    for (int k = 0; k < 3; k++) {
      const RingElem t = ds[k]->to_poly();
      dd[k] = upload_words(t.get_poly());
      dp[k] = dd[k].get();
    }
  }
  rs_rinocchio_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.alpha_s_pows = pk.alpha_s_pows_.get(), k.beta_prods = pk.beta_prods_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_beta_rv_ts = pk.beta_rv_ts_.get(), k.d_beta_rw_ts = pk.beta_rw_ts_.get(), k.d_beta_ry_ts = pk.beta_ry_ts_.get();
  int empty[9] = {0};
  const std::vector<uint8_t> kinds = wire_kinds(full);
  check(rs_rinocchio_prove_seeded(Context::get_context(), pk.cs.get(), &k, dasg.get(), kinds.data(), dp[0], dp[1], dp[2], dproof.get(), empty,
                                  nullptr));
  std::vector<uint64_t> w(9 * Context::enc_words());
  dproof.download(w.data());
  proof p;
  EncodingElem *dst[9] = {&p.A, &p.A_prime, &p.B, &p.B_prime, &p.C, &p.C_prime, &p.D, &p.D_prime, &p.F};
  for (int i = 0; i < 9; i++)
    if (!empty[i]) *dst[i] = take_element(w, i);
  return p;
}
inline proof prover(const seeded_proving_key &pk, const std::vector<RingElem> &primary_input,
                    const std::vector<RingElem> &auxiliary_input) {
  if (auxiliary_input.empty()) {
    std::cout << "[Prover] using non-zero-knowledge SNARK, since no auxiliary inputs are defined" << std::endl;  // rinocchio.tcc:82-87
    return prover(pk, primary_input, auxiliary_input, nullptr, nullptr, nullptr);
  }
  const RingElem d1 = RingElem::random_invertible_element(), d2 = RingElem::random_invertible_element(),
                 d3 = RingElem::random_invertible_element();
  return prover(pk, primary_input, auxiliary_input, &d1, &d2, &d3);
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
