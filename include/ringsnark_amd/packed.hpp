// packed.hpp -- header-only C++ adapter of bit-packed seeded proving keys (packed.h) on the types of ring.hpp, keygen.hpp,
// seeded.hpp and batch.hpp.  A header of its own, beside seeded.hpp, for the reason given in r1cs_check.h: the adapters that
// exist stay as they are.
//
// generator(cs, packed) -- the tag `ringsnark::amd::packed` after the constraint system -- samples the trapdoor and the seeds
// as generator(cs, seeded) of seeded.hpp does and returns {packed_proving_key, verification_key}: the three vectors of the
// key are [count][L][K][row_words] words (packed.h), w / 64 of the seeded key's device memory.  prover(pk, ...) and
// prove_batch(pk, ...) on a packed_proving_key call the _packed entry points.  A packed_proving_key is a type of its own, not
// a seeded_proving_key: the provers of seeded.hpp would read its vectors as compact ones.
#ifndef RINGSNARK_AMD_PACKED_HPP
#define RINGSNARK_AMD_PACKED_HPP

#include <algorithm>

#include "batch.hpp"
#include "packed.h"

namespace ringsnark::amd {

struct packed_t {};
inline constexpr packed_t packed{};

// words of one packed element of the current context
inline size_t packed_words() { return rs_enc_packed_words(Context::get_context()); }

namespace groth16 {
// s_pows_, delta_ts_, delta_mid_ are PACKED [count][L][K][row_words]; alpha_, beta_ full elements
struct packed_proving_key : generated_proving_key {
  packed_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords delta_ts, DeviceWords delta_mid, DeviceWords alpha,
                     DeviceWords beta, const uint64_t (&pub)[5])
      : generated_proving_key(cs_, std::move(s_pows), std::move(delta_ts), std::move(delta_mid), std::move(alpha), std::move(beta)) {
    std::copy(pub, pub + 5, pub_seeds);
  }
  uint64_t pub_seeds[5];  // of s_pows, delta_ts, delta_mid, alpha, beta
};
struct packed_keypair {
  packed_proving_key pk;
  verification_key vk;
};
// groth16::generator (groth16.tcc:5-66) with a packed proving key
inline packed_keypair generator(const R1csCsr &cs, packed_t) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words(), pw = packed_words();
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
  DeviceWords s_pows((m + 1) * pw), delta_ts((m + 1) * pw), delta_mid(n_aux * pw), ealpha(ew), ebeta(ew);
  rs_groth16_seeded_key_out out{};
  out.s_pows = s_pows.get(), out.delta_ts = delta_ts.get(), out.delta_mid = delta_mid.get();
  out.d_alpha = ealpha.get(), out.d_beta = ebeta.get();
  check(rs_groth16_keygen_packed(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), ddelta.get(), dsk.get(), seeds,
                                 pub, &out, nullptr));
  return packed_keypair{packed_proving_key(cs, std::move(s_pows), std::move(delta_ts), std::move(delta_mid), std::move(ealpha),
                                           std::move(ebeta), pub),
                        verification_key{cs, s, alpha, beta, gamma, delta, sk}};
}
namespace detail_packed {
inline rs_groth16_pk_seeded key_struct(const packed_proving_key &pk) {
  rs_groth16_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.delta_ts = pk.delta_ts_.get(), k.delta_mid = pk.delta_mid_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_alpha = pk.alpha_.get(), k.d_beta = pk.beta_.get();
  return k;
}
}  // namespace detail_packed
// groth16::prover (groth16.tcc:70-115) on a packed key
inline proof prover(const packed_proving_key &pk, const std::vector<RingElem> &primary_input,
                    const std::vector<RingElem> &auxiliary_input) {
  if (primary_input.size() != pk.cs.n_inputs || primary_input.size() + auxiliary_input.size() != pk.cs.n_vars)
    throw std::invalid_argument("assignment does not match the constraint system");
  std::vector<RingElem> full(primary_input);
  full.insert(full.end(), auxiliary_input.begin(), auxiliary_input.end());
  const std::vector<uint64_t> asg = flatten(full);
  DeviceWords dasg(asg.data(), asg.size()), dproof(3 * Context::enc_words());
  const rs_groth16_pk_seeded k = detail_packed::key_struct(pk);
  int empty[3] = {0, 0, 0};
  const std::vector<uint8_t> kinds = wire_kinds(full);
  check(rs_groth16_prove_packed(Context::get_context(), pk.cs.get(), &k, dasg.get(), kinds.data(), dproof.get(), empty, nullptr));
  std::vector<uint64_t> w(3 * Context::enc_words());
  dproof.download(w.data());
  proof p;
  EncodingElem *dst[3] = {&p.A, &p.B, &p.C};
  for (int i = 0; i < 3; i++)
    if (!empty[i]) *dst[i] = take_element(w, i);
  return p;
}
inline std::vector<proof> prove_batch(const packed_proving_key &pk, const std::vector<batch_input> &inputs) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  DeviceWords dproofs((size_t)3 * B * Context::enc_words());
  std::vector<int> empty((size_t)3 * B, 0);
  const rs_groth16_pk_seeded k = detail_packed::key_struct(pk);
  check(rs_groth16_prove_batch_packed(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(), dproofs.get(),
                                      empty.data(), nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
}  // namespace groth16

namespace rinocchio {
// as groth16::packed_proving_key: s_pows_, alpha_s_pows_, beta_prods_ packed
struct packed_proving_key : generated_proving_key {
  packed_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords alpha_s_pows, DeviceWords beta_prods, DeviceWords beta_rv_ts,
                     DeviceWords beta_rw_ts, DeviceWords beta_ry_ts, const uint64_t (&pub)[6])
      : generated_proving_key(cs_, std::move(s_pows), std::move(alpha_s_pows), std::move(beta_prods), std::move(beta_rv_ts),
                              std::move(beta_rw_ts), std::move(beta_ry_ts)) {
    std::copy(pub, pub + 6, pub_seeds);
  }
  uint64_t pub_seeds[6];  // of s_pows, alpha_s_pows, beta_prods, beta_rv_ts, beta_rw_ts, beta_ry_ts
};
struct packed_keypair {
  packed_proving_key pk;
  verification_key vk;
};
// rinocchio::generator (rinocchio.tcc:5-72) with a packed proving key
inline packed_keypair generator(const R1csCsr &cs, packed_t) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words(), pw = packed_words();
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
  DeviceWords s_pows((m + 1) * pw), alpha_s_pows((m + 1) * pw), beta_prods(n_aux * pw), rv_ts(ew), rw_ts(ew), ry_ts(ew);
  rs_rinocchio_seeded_key_out out{};
  out.s_pows = s_pows.get(), out.alpha_s_pows = alpha_s_pows.get(), out.beta_prods = beta_prods.get();
  out.d_beta_rv_ts = rv_ts.get(), out.d_beta_rw_ts = rw_ts.get(), out.d_beta_ry_ts = ry_ts.get();
  check(rs_rinocchio_keygen_packed(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), drv.get(), drw.get(), dry.get(),
                                   dsk.get(), seeds, pub, &out, nullptr));
  return packed_keypair{packed_proving_key(cs, std::move(s_pows), std::move(alpha_s_pows), std::move(beta_prods), std::move(rv_ts),
                                           std::move(rw_ts), std::move(ry_ts), pub),
                        verification_key{cs, s, alpha, beta, r_v, r_w, r_y, sk}};
}
namespace detail_packed {
inline rs_rinocchio_pk_seeded key_struct(const packed_proving_key &pk) {
  rs_rinocchio_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.alpha_s_pows = pk.alpha_s_pows_.get(), k.beta_prods = pk.beta_prods_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_beta_rv_ts = pk.beta_rv_ts_.get(), k.d_beta_rw_ts = pk.beta_rw_ts_.get(), k.d_beta_ry_ts = pk.beta_ry_ts_.get();
  return k;
}
}  // namespace detail_packed
// rinocchio::prover (rinocchio.tcc:75-190) on a packed key; d1, d2, d3 as in ring.hpp
inline proof prover(const packed_proving_key &pk, const std::vector<RingElem> &primary_input,
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
  const rs_rinocchio_pk_seeded k = detail_packed::key_struct(pk);
  int empty[9] = {0};
  const std::vector<uint8_t> kinds = wire_kinds(full);
  check(rs_rinocchio_prove_packed(Context::get_context(), pk.cs.get(), &k, dasg.get(), kinds.data(), dp[0], dp[1], dp[2], dproof.get(), empty,
                                  nullptr));
  std::vector<uint64_t> w(9 * Context::enc_words());
  dproof.download(w.data());
  proof p;
  EncodingElem *dst[9] = {&p.A, &p.A_prime, &p.B, &p.B_prime, &p.C, &p.C_prime, &p.D, &p.D_prime, &p.F};
  for (int i = 0; i < 9; i++)
    if (!empty[i]) *dst[i] = take_element(w, i);
  return p;
}
inline proof prover(const packed_proving_key &pk, const std::vector<RingElem> &primary_input,
                    const std::vector<RingElem> &auxiliary_input) {
  if (auxiliary_input.empty()) {
    std::cout << "[Prover] using non-zero-knowledge SNARK, since no auxiliary inputs are defined" << std::endl;  // rinocchio.tcc:82-87
    return prover(pk, primary_input, auxiliary_input, nullptr, nullptr, nullptr);
  }
  const RingElem d1 = RingElem::random_invertible_element(), d2 = RingElem::random_invertible_element(),
                 d3 = RingElem::random_invertible_element();
  return prover(pk, primary_input, auxiliary_input, &d1, &d2, &d3);
}
// d: the blinding elements of every member, or nullptr: non-ZK proofs
inline std::vector<proof> prove_batch(const packed_proving_key &pk, const std::vector<batch_input> &inputs, const std::vector<blinding> *d) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  const DeviceWords dd = detail_batch::upload_blinding(d, B);
  DeviceWords dproofs((size_t)9 * B * Context::enc_words());
  std::vector<int> empty((size_t)9 * B, 0);
  const rs_rinocchio_pk_seeded k = detail_packed::key_struct(pk);
  check(rs_rinocchio_prove_batch_packed(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(),
                                        d ? dd.get() : nullptr, dproofs.get(), empty.data(), nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
