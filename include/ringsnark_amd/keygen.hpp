// keygen.hpp -- header-only C++ adapter of the device generators (keygen.h) on the types of ring.hpp and verify.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes verify.hpp, so one include gives all three.
//
// The reference's generator<RingT, EncT>(cs) (zk_proof_systems/groth16/groth16.tcc:5-66,
// zk_proof_systems/rinocchio/rinocchio.tcc:5-72) returns keypair{pk, vk}.  Here the trapdoor is sampled on the host exactly
// as there -- RingElem::random_exceptional_element(domain), random_invertible_element, random_nonzero_element and
// EncodingElem::keygen, all on the context's ChaCha20 generator -- and the proving key is made on the device and stays
// there: generator(cs) returns {generated_proving_key (a proving_key_device), verification_key}, ready for prover(pk, ...) and verifier(vk, ...).
// The per-vector seeds are disjoint stream ranges drawn from the same generator (keygen.h "Randomness").
#ifndef RINGSNARK_AMD_KEYGEN_HPP
#define RINGSNARK_AMD_KEYGEN_HPP

#include <memory>

#include "keygen.h"
#include "verify.hpp"

namespace ringsnark::amd {

namespace detail {
struct keygen_domain {  // what random_exceptional_element reads of evaluation_domain<RingT>
  size_t m;
};
inline RingElem random_point(size_t m) { return RingElem::random_exceptional_element(std::make_shared<keygen_domain>(keygen_domain{m})); }
// n seeds whose ranges [seed, seed + 2^40) cannot meet: the top 20 bits are random and shared, the next four number the vector
template <size_t NV>
inline void keygen_seeds(uint64_t (&seeds)[NV]) {
  static_assert(NV <= 16, "four bits number the vectors");
  const uint64_t base = Context::prng()() & ~((uint64_t(1) << 44) - 1);
  for (size_t v = 0; v < NV; v++) seeds[v] = base | ((uint64_t)v << 40) | (Context::prng()() & ((uint64_t(1) << 39) - 1));
}
}  // namespace detail

namespace groth16 {
// A proving_key_device whose vectors were made on the device: it adopts the buffers, no host round trip.  (A type of this
// header, not a constructor of proving_key_device: ring.hpp stays as it is for the reason given in r1cs_check.h.)
// prover(const proving_key_device &, ...) takes it as it is.
struct generated_proving_key : proving_key_device {
  generated_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords delta_ts, DeviceWords delta_mid, DeviceWords alpha,
                        DeviceWords beta)
      : proving_key_device(cs_, std::vector<EncodingElem>(), std::vector<EncodingElem>(), std::vector<EncodingElem>(), EncodingElem(),
                           EncodingElem()) {
    s_pows_ = std::move(s_pows), delta_ts_ = std::move(delta_ts), delta_mid_ = std::move(delta_mid);
    alpha_ = std::move(alpha), beta_ = std::move(beta);
  }
};
struct keypair {
  generated_proving_key pk;
  verification_key vk;
};
// groth16::generator (groth16.tcc:5-66)
inline keypair generator(const R1csCsr &cs) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words();
  const RingElem s = detail::random_point(m);
  const EncodingElem::SecretKey sk = std::get<1>(EncodingElem::keygen());
  const RingElem alpha = RingElem::random_invertible_element(), beta = RingElem::random_invertible_element(),
                 gamma = RingElem::random_invertible_element(), delta = RingElem::random_invertible_element();
  uint64_t seeds[5];
  detail::keygen_seeds(seeds);
  const DeviceR1cs dcs(cs);
  const DeviceWords ds = detail::upload_ring(s), dalpha = detail::upload_ring(alpha), dbeta = detail::upload_ring(beta),
                    ddelta = detail::upload_ring(delta), dsk = upload_words(sk);
  DeviceWords s_pows((m + 1) * ew), delta_ts((m + 1) * ew), delta_mid(n_aux * ew), ealpha(ew), ebeta(ew);
  rs_groth16_key_out out{};
  out.s_pows = s_pows.get(), out.delta_ts = delta_ts.get(), out.delta_mid = delta_mid.get();
  out.d_alpha = ealpha.get(), out.d_beta = ebeta.get();
  check(rs_groth16_keygen(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), ddelta.get(), dsk.get(), seeds, &out,
                          nullptr));
  return keypair{generated_proving_key(cs, std::move(s_pows), std::move(delta_ts), std::move(delta_mid), std::move(ealpha), std::move(ebeta)),
                 verification_key{cs, s, alpha, beta, gamma, delta, sk}};
}
}  // namespace groth16

namespace rinocchio {
// as groth16::generated_proving_key
struct generated_proving_key : proving_key_device {
  generated_proving_key(const R1csCsr &cs_, DeviceWords s_pows, DeviceWords alpha_s_pows, DeviceWords beta_prods, DeviceWords beta_rv_ts,
                        DeviceWords beta_rw_ts, DeviceWords beta_ry_ts)
      : proving_key_device(cs_, std::vector<EncodingElem>(), std::vector<EncodingElem>(), std::vector<EncodingElem>(), EncodingElem(),
                           EncodingElem(), EncodingElem()) {
    s_pows_ = std::move(s_pows), alpha_s_pows_ = std::move(alpha_s_pows), beta_prods_ = std::move(beta_prods);
    beta_rv_ts_ = std::move(beta_rv_ts), beta_rw_ts_ = std::move(beta_rw_ts), beta_ry_ts_ = std::move(beta_ry_ts);
  }
};
struct keypair {
  generated_proving_key pk;
  verification_key vk;
};
// rinocchio::generator (rinocchio.tcc:5-72)
inline keypair generator(const R1csCsr &cs) {
  const size_t m = cs.m, n_aux = cs.n_vars - cs.n_inputs, ew = Context::enc_words();
  const RingElem s = detail::random_point(m);
  const EncodingElem::SecretKey sk = std::get<1>(EncodingElem::keygen());
  const RingElem alpha = RingElem::random_invertible_element(), r_v = RingElem::random_invertible_element(),
                 r_w = RingElem::random_invertible_element(), r_y = r_v * r_w, beta = RingElem::random_nonzero_element();
  uint64_t seeds[6];
  detail::keygen_seeds(seeds);
  const DeviceR1cs dcs(cs);
  const DeviceWords ds = detail::upload_ring(s), dalpha = detail::upload_ring(alpha), dbeta = detail::upload_ring(beta),
                    drv = detail::upload_ring(r_v), drw = detail::upload_ring(r_w), dry = detail::upload_ring(r_y), dsk = upload_words(sk);
  DeviceWords s_pows((m + 1) * ew), alpha_s_pows((m + 1) * ew), beta_prods(n_aux * ew), rv_ts(ew), rw_ts(ew), ry_ts(ew);
  rs_rinocchio_key_out out{};
  out.s_pows = s_pows.get(), out.alpha_s_pows = alpha_s_pows.get(), out.beta_prods = beta_prods.get();
  out.d_beta_rv_ts = rv_ts.get(), out.d_beta_rw_ts = rw_ts.get(), out.d_beta_ry_ts = ry_ts.get();
  check(rs_rinocchio_keygen(Context::get_context(), dcs.get(), ds.get(), dalpha.get(), dbeta.get(), drv.get(), drw.get(), dry.get(),
                            dsk.get(), seeds, &out, nullptr));
  return keypair{generated_proving_key(cs, std::move(s_pows), std::move(alpha_s_pows), std::move(beta_prods), std::move(rv_ts),
                                    std::move(rw_ts), std::move(ry_ts)),
                 verification_key{cs, s, alpha, beta, r_v, r_w, r_y, sk}};
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
