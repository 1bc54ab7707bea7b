// verify.hpp -- header-only C++ adapter of the device verifiers (verify.h) on the types of ring.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
//
// The reference's verifier<RingT, EncT>(vk, primary_input, proof) (zk_proof_systems/groth16/groth16.tcc:117-170,
// zk_proof_systems/rinocchio/rinocchio.tcc:192-295) recomputes the instance map at vk.s for every proof.  Here the key is
// put on the device once (verification_key_device: rs_*_vk_create evaluates the public columns at s) and a verification
// is a decode plus one kernel; verifier(vk, ...) on the plain key struct does both for one call, as the reference does.
#ifndef RINGSNARK_AMD_VERIFY_HPP
#define RINGSNARK_AMD_VERIFY_HPP

#include "ring.hpp"
#include "verify.h"

namespace ringsnark::amd {

namespace detail {
inline DeviceWords upload_ring(const RingElem &r) { return upload_words(r.to_poly().get_poly()); }
inline DeviceWords upload_primary(const std::vector<RingElem> &primary_input) {
  if (primary_input.empty()) return DeviceWords();
  const std::vector<uint64_t> w = flatten(primary_input);
  return DeviceWords(w.data(), w.size());
}
// the proof's elements side by side, EMPTY ones (seal_ring.hpp:243,249) as zeros with their flag set
template <size_t NE>
inline DeviceWords upload_proof(const EncodingElem *const (&elems)[NE], int (&empty)[NE]) {
  const size_t ew = Context::enc_words();
  std::vector<uint64_t> w(NE * ew, 0);
  for (size_t k = 0; k < NE; k++) {
    empty[k] = elems[k]->is_empty() ? 1 : 0;
    if (!empty[k]) std::memcpy(&w[k * ew], elems[k]->words().data(), ew * 8);
  }
  return DeviceWords(w.data(), w.size());
}
}  // namespace detail

namespace groth16 {
// verification_key (zk_proof_systems/groth16/groth16.hpp:50-86): the reference's members; its `pk` is kept for the
// constraint system alone (vk.pk.constraint_system, groth16.tcc:125), which is what this struct holds.
struct verification_key {
  R1csCsr constraint_system;
  RingElem s, alpha, beta, gamma, delta;
  EncodingElem::SecretKey sk_enc;
};
// the key on the device.  Throws std::invalid_argument("element is not invertible in ring") unless gamma is a unit
// (groth16.tcc:162 divides by it) and when s is a domain element (util/evaluation_domain.tcc:24-26).
class verification_key_device {
 public:
  explicit verification_key_device(const verification_key &vk) : n_inputs(vk.constraint_system.n_inputs) {
    const DeviceR1cs cs(vk.constraint_system);
    const DeviceWords s = detail::upload_ring(vk.s), alpha = detail::upload_ring(vk.alpha), beta = detail::upload_ring(vk.beta),
                      gamma = detail::upload_ring(vk.gamma), delta = detail::upload_ring(vk.delta), sk = upload_words(vk.sk_enc);
    check(rs_groth16_vk_create(Context::get_context(), cs.get(), s.get(), alpha.get(), beta.get(), gamma.get(), delta.get(), sk.get(), &h_));
  }
  ~verification_key_device() { rs_groth16_vk_destroy(h_); }
  verification_key_device(const verification_key_device &) = delete;
  const rs_groth16_vk *get() const { return h_; }
  size_t n_inputs;

 private:
  rs_groth16_vk *h_ = nullptr;
};
// groth16::verifier (groth16.tcc:117-170).  Throws decoding_error when a proof element's noise budget is spent, as the
// reference's EncT::decode does (seal_ring.tcc:446-454); `report` says which positions fail and with which residues.
inline bool verifier(const verification_key_device &vk, const std::vector<RingElem> &primary_input, const proof &proof,
                     rs_verify_report *report = nullptr) {
  if (primary_input.size() != vk.n_inputs) throw std::invalid_argument("primary input does not match the constraint system");
  const EncodingElem *const elems[3] = {&proof.A, &proof.B, &proof.C};
  int empty[3];
  const DeviceWords dproof = detail::upload_proof(elems, empty), dprimary = detail::upload_primary(primary_input);
  rs_verify_report rep;
  check(rs_groth16_verify(Context::get_context(), vk.get(), dprimary.get(), dproof.get(), empty, &rep, nullptr));
  if (report) *report = rep;
  return rep.accepted != 0;
}
inline bool verifier(const verification_key &vk, const std::vector<RingElem> &primary_input, const proof &proof) {
  return verifier(verification_key_device(vk), primary_input, proof);
}
}  // namespace groth16

namespace rinocchio {
// verification_key (zk_proof_systems/rinocchio/rinocchio.hpp:60-97)
struct verification_key {
  R1csCsr constraint_system;
  RingElem s, alpha, beta, r_v, r_w, r_y;
  EncodingElem::SecretKey sk_enc;
};
class verification_key_device {
 public:
  explicit verification_key_device(const verification_key &vk) : n_inputs(vk.constraint_system.n_inputs) {
    const DeviceR1cs cs(vk.constraint_system);
    const DeviceWords s = detail::upload_ring(vk.s), alpha = detail::upload_ring(vk.alpha), beta = detail::upload_ring(vk.beta),
                      rv = detail::upload_ring(vk.r_v), rw = detail::upload_ring(vk.r_w), ry = detail::upload_ring(vk.r_y),
                      sk = upload_words(vk.sk_enc);
    check(rs_rinocchio_vk_create(Context::get_context(), cs.get(), s.get(), alpha.get(), beta.get(), rv.get(), rw.get(), ry.get(), sk.get(), &h_));
  }
  ~verification_key_device() { rs_rinocchio_vk_destroy(h_); }
  verification_key_device(const verification_key_device &) = delete;
  const rs_rinocchio_vk *get() const { return h_; }
  size_t n_inputs;

 private:
  rs_rinocchio_vk *h_ = nullptr;
};
// rinocchio::verifier (rinocchio.tcc:192-295): the six checks; an EMPTY last element (no auxiliary inputs, :199-206)
// skips the L_beta check (:283-288).  report->failed has bit c set for check c of verify.h.
inline bool verifier(const verification_key_device &vk, const std::vector<RingElem> &primary_input, const proof &proof,
                     rs_verify_report *report = nullptr) {
  if (primary_input.size() != vk.n_inputs) throw std::invalid_argument("primary input does not match the constraint system");
  const EncodingElem *const elems[9] = {&proof.A, &proof.A_prime, &proof.B, &proof.B_prime, &proof.C,
                                        &proof.C_prime, &proof.D, &proof.D_prime, &proof.F};
  int empty[9];
  const DeviceWords dproof = detail::upload_proof(elems, empty), dprimary = detail::upload_primary(primary_input);
  rs_verify_report rep;
  check(rs_rinocchio_verify(Context::get_context(), vk.get(), dprimary.get(), dproof.get(), empty, &rep, nullptr));
  if (report) *report = rep;
  return rep.accepted != 0;
}
inline bool verifier(const verification_key &vk, const std::vector<RingElem> &primary_input, const proof &proof) {
  return verifier(verification_key_device(vk), primary_input, proof);
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
