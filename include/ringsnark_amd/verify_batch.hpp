// verify_batch.hpp -- header-only C++ adapter of batched verification (verify_batch.h) on the types of ring.hpp, verify.hpp
// and modswitch.hpp.  A header of its own, as batch.hpp is; it includes modswitch.hpp, so one include gives all of them.
//
// The reference verifies one proof per call (zk_proof_systems/groth16/groth16.tcc:117-170,
// zk_proof_systems/rinocchio/rinocchio.tcc:192-295).  verify_batch(vk, primary_inputs, proofs) gives, for every member, what
// verifier(vk, primary_inputs[b], proofs[b], &report) gives -- the same report in every field -- in one decode and one pass
// over the key's public columns per RS_VERIFY_BATCH_MAX members.  Where the single verifier throws decoding_error (a spent
// noise budget, seal_ring.tcc:446-454) the member's verdict says noise_spent and the others are not affected.
#ifndef RINGSNARK_AMD_VERIFY_BATCH_HPP
#define RINGSNARK_AMD_VERIFY_BATCH_HPP

#include <algorithm>
#include <array>

#include "modswitch.hpp"
#include "verify_batch.h"

namespace ringsnark::amd {

struct batch_verdict {
  bool noise_spent = false;   // the single verifier throws decoding_error for this member; report is all zero
  int budget_min = 0;         // smallest noise budget over the member's non-EMPTY ciphertexts (verify_batch.h)
  rs_verify_report report{};  // what verifier(vk, primary_input, proof, &report) reports
  bool accepted() const { return !noise_spent && report.accepted != 0; }
};

namespace detail {
// words(e): the payload of element e or nullptr for an EMPTY one; call: the C entry point of the scheme
template <size_t NE, class Proof, class Elems, class Words, class Call>
inline std::vector<batch_verdict> verify_batch_chunks(size_t n_inputs, const std::vector<std::vector<RingElem>> &primary_inputs,
                                                      const std::vector<Proof> &proofs, size_t elem_words, Elems &&elems, Words &&words,
                                                      Call &&call) {
  if (primary_inputs.size() != proofs.size()) throw std::invalid_argument("as many primary inputs as proofs");
  for (const auto &x : primary_inputs)
    if (x.size() != n_inputs) throw std::invalid_argument("primary input does not match the constraint system");
  std::vector<batch_verdict> out;
  out.reserve(proofs.size());
  for (size_t b0 = 0; b0 < proofs.size(); b0 += RS_VERIFY_BATCH_MAX) {
    const size_t nb = std::min<size_t>(RS_VERIFY_BATCH_MAX, proofs.size() - b0);
    std::vector<uint64_t> pw(nb * NE * elem_words, 0), xw;
    std::vector<int> empty(nb * NE), status(nb), budget(nb);
    std::vector<rs_verify_report> reports(nb);
    for (size_t b = 0; b < nb; b++) {
      const auto el = elems(proofs[b0 + b]);
      for (size_t k = 0; k < NE; k++) {
        const uint64_t *w = words(*el[k]);
        empty[b * NE + k] = w ? 0 : 1;
        if (w) std::memcpy(&pw[(b * NE + k) * elem_words], w, elem_words * 8);
      }
      const std::vector<uint64_t> x = flatten(primary_inputs[b0 + b]);
      xw.insert(xw.end(), x.begin(), x.end());
    }
    const DeviceWords dproofs(pw.data(), pw.size()), dprimary(xw.data(), xw.size());  // no inputs: no words, a null pointer
    check(call((int)nb, dprimary.get(), dproofs.get(), empty.data(), status.data(), budget.data(), reports.data()));
    for (size_t b = 0; b < nb; b++) {
      batch_verdict v;
      v.noise_spent = status[b] == RS_ERR_NOISE;
      v.budget_min = budget[b];
      v.report = reports[b];
      out.push_back(v);
    }
  }
  return out;
}
inline const uint64_t *words_of(const EncodingElem &e) { return e.is_empty() ? nullptr : e.words().data(); }
// a switched element must be of the batch's level
inline auto words_at_level(int K_lvl) {
  return [K_lvl](const SwitchedEncodingElem &e) -> const uint64_t * {
    if (e.is_empty()) return nullptr;
    if (e.level() != K_lvl) throw std::invalid_argument("proof elements of different levels");
    return e.words().data();
  };
}
}  // namespace detail

namespace groth16 {
namespace detail_batch {
template <class P>
inline std::array<const decltype(P::A) *, 3> elems(const P &p) { return {&p.A, &p.B, &p.C}; }
inline auto call(const verification_key_device &vk, int K_lvl) {
  return [&vk, K_lvl](int nb, const uint64_t *x, const uint64_t *p, const int *em, int *st, int *bu, rs_verify_report *rep) {
    return rs_groth16_verify_batch(Context::get_context(), vk.get(), K_lvl, nb, x, p, em, st, bu, rep, nullptr);
  };
}
}  // namespace detail_batch
inline std::vector<batch_verdict> verify_batch(const verification_key_device &vk, const std::vector<std::vector<RingElem>> &primary_inputs,
                                               const std::vector<proof> &proofs) {
  return detail::verify_batch_chunks<3>(vk.n_inputs, primary_inputs, proofs, Context::enc_words(), detail_batch::elems<proof>,
                                        detail::words_of, detail_batch::call(vk, Context::get_params().K));
}
// proofs switched to K_lvl primes (modswitch.hpp)
inline std::vector<batch_verdict> verify_batch(const verification_key_device &vk, const std::vector<std::vector<RingElem>> &primary_inputs,
                                               const std::vector<switched_proof> &proofs, int K_lvl) {
  return detail::verify_batch_chunks<3>(vk.n_inputs, primary_inputs, proofs, SwitchedEncodingElem::level_words(K_lvl),
                                        detail_batch::elems<switched_proof>, detail::words_at_level(K_lvl), detail_batch::call(vk, K_lvl));
}
}  // namespace groth16

namespace rinocchio {
namespace detail_batch {
template <class P>
inline std::array<const decltype(P::A) *, 9> elems(const P &p) {
  return {&p.A, &p.A_prime, &p.B, &p.B_prime, &p.C, &p.C_prime, &p.D, &p.D_prime, &p.F};
}
inline auto call(const verification_key_device &vk, int K_lvl) {
  return [&vk, K_lvl](int nb, const uint64_t *x, const uint64_t *p, const int *em, int *st, int *bu, rs_verify_report *rep) {
    return rs_rinocchio_verify_batch(Context::get_context(), vk.get(), K_lvl, nb, x, p, em, st, bu, rep, nullptr);
  };
}
}  // namespace detail_batch
// a member whose F is EMPTY skips the L_beta check, its neighbours do not (rinocchio.tcc:199-206, 283-288)
inline std::vector<batch_verdict> verify_batch(const verification_key_device &vk, const std::vector<std::vector<RingElem>> &primary_inputs,
                                               const std::vector<proof> &proofs) {
  return detail::verify_batch_chunks<9>(vk.n_inputs, primary_inputs, proofs, Context::enc_words(), detail_batch::elems<proof>,
                                        detail::words_of, detail_batch::call(vk, Context::get_params().K));
}
inline std::vector<batch_verdict> verify_batch(const verification_key_device &vk, const std::vector<std::vector<RingElem>> &primary_inputs,
                                               const std::vector<switched_proof> &proofs, int K_lvl) {
  return detail::verify_batch_chunks<9>(vk.n_inputs, primary_inputs, proofs, SwitchedEncodingElem::level_words(K_lvl),
                                        detail_batch::elems<switched_proof>, detail::words_at_level(K_lvl), detail_batch::call(vk, K_lvl));
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
