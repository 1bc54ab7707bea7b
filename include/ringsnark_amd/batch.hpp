// batch.hpp -- header-only C++ adapter of batched proving (batch.h) on the types of ring.hpp, keygen.hpp and seeded.hpp.
// A header of its own, beside seeded.hpp, for the reason given in r1cs_check.h: the adapters that exist stay as they are.
//
// prove_batch(pk, inputs) proves every (primary, auxiliary) input of `inputs` -- statements of ONE constraint system --
// against one key in one pass over every key vector, and returns the proofs in the order of the inputs.  Proof b is what
// prover(pk, inputs[b].primary, inputs[b].auxiliary) returns (for Rinocchio: with the same blinding elements).  pk is a
// proving_key_device (ring.hpp, keygen.hpp) or a seeded_proving_key (seeded.hpp).  1 <= inputs.size() <= RS_MAX_BATCH.
#ifndef RINGSNARK_AMD_BATCH_HPP
#define RINGSNARK_AMD_BATCH_HPP

#include <array>

#include "batch.h"
#include "seeded.hpp"

namespace ringsnark::amd {

struct batch_input {
  std::vector<RingElem> primary, auxiliary;
};

namespace detail {
// the members' assignments on the device, their wire kinds [B][n_vars] and the host array of device pointers
struct BatchAssignments {
  std::vector<DeviceWords> words;
  std::vector<const uint64_t *> ptrs;
  std::vector<uint8_t> kinds;
  BatchAssignments(const DeviceR1cs &cs, const std::vector<batch_input> &inputs) {
    if (inputs.empty() || inputs.size() > RS_MAX_BATCH) throw std::invalid_argument("batch size out of range");
    for (const batch_input &in : inputs) {
      if (in.primary.size() != cs.n_inputs || in.primary.size() + in.auxiliary.size() != cs.n_vars)
        throw std::invalid_argument("assignment does not match the constraint system");
      std::vector<RingElem> full(in.primary);
      full.insert(full.end(), in.auxiliary.begin(), in.auxiliary.end());
      const std::vector<uint64_t> asg = flatten(full);
      words.emplace_back(asg.data(), asg.size());
      ptrs.push_back(words.back().get());
      const std::vector<uint8_t> k = wire_kinds(full);
      kinds.insert(kinds.end(), k.begin(), k.end());
    }
  }
  int size() const { return (int)ptrs.size(); }
};
}  // namespace detail

namespace groth16 {
namespace detail_batch {
inline std::vector<proof> take_proofs(const DeviceWords &dproofs, const std::vector<int> &empty, int B) {
  std::vector<uint64_t> w(dproofs.words());
  dproofs.download(w.data());
  std::vector<proof> out((size_t)B);
  for (int b = 0; b < B; b++) {
    EncodingElem *dst[3] = {&out[b].A, &out[b].B, &out[b].C};
    for (int i = 0; i < 3; i++)
      if (!empty[3 * b + i]) *dst[i] = take_element(w, (size_t)3 * b + i);
  }
  return out;
}
}  // namespace detail_batch
inline std::vector<proof> prove_batch(const proving_key_device &pk, const std::vector<batch_input> &inputs) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  DeviceWords dproofs((size_t)3 * B * Context::enc_words());
  std::vector<int> empty((size_t)3 * B, 0);
  rs_groth16_pk k{pk.s_pows_.get(), pk.delta_ts_.get(), pk.delta_mid_.get(), pk.alpha_.get(), pk.beta_.get(), 0, 0};
  check(rs_groth16_prove_batch(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(), dproofs.get(), empty.data(),
                               nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
inline std::vector<proof> prove_batch(const seeded_proving_key &pk, const std::vector<batch_input> &inputs) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  DeviceWords dproofs((size_t)3 * B * Context::enc_words());
  std::vector<int> empty((size_t)3 * B, 0);
  rs_groth16_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.delta_ts = pk.delta_ts_.get(), k.delta_mid = pk.delta_mid_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_alpha = pk.alpha_.get(), k.d_beta = pk.beta_.get();
  check(rs_groth16_prove_batch_seeded(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(), dproofs.get(),
                                      empty.data(), nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
}  // namespace groth16

namespace rinocchio {
using blinding = std::array<RingElem, 3>;  // d1, d2, d3 of one member
namespace detail_batch {
// [B][3][L][N] on the device, or an empty buffer for a non-ZK batch
inline DeviceWords upload_blinding(const std::vector<blinding> *d, int B) {
  if (!d) return DeviceWords();
  if ((int)d->size() != B) throw std::invalid_argument("one (d1, d2, d3) per member");
  std::vector<uint64_t> w;
  for (const blinding &t : *d)
    for (const RingElem &e : t) {
      const RingElem p = e.to_poly();
      w.insert(w.end(), p.get_poly().begin(), p.get_poly().end());
    }
  return upload_words(w);
}
inline std::vector<proof> take_proofs(const DeviceWords &dproofs, const std::vector<int> &empty, int B) {
  std::vector<uint64_t> w(dproofs.words());
  dproofs.download(w.data());
  std::vector<proof> out((size_t)B);
  for (int b = 0; b < B; b++) {
    proof &p = out[b];
    EncodingElem *dst[9] = {&p.A, &p.A_prime, &p.B, &p.B_prime, &p.C, &p.C_prime, &p.D, &p.D_prime, &p.F};
    for (int i = 0; i < 9; i++)
      if (!empty[9 * b + i]) *dst[i] = take_element(w, (size_t)9 * b + i);
  }
  return out;
}
// the blinding elements the reference's prover samples (rinocchio.tcc:81-90), per member
inline std::vector<blinding> sample_blinding(size_t B) {
  std::vector<blinding> d;
  for (size_t b = 0; b < B; b++)
    d.push_back(blinding{RingElem::random_invertible_element(), RingElem::random_invertible_element(), RingElem::random_invertible_element()});
  return d;
}
}  // namespace detail_batch
// d: the blinding elements of every member, or nullptr: non-ZK proofs (prover(pk, ..., nullptr, nullptr, nullptr))
inline std::vector<proof> prove_batch(const proving_key_device &pk, const std::vector<batch_input> &inputs, const std::vector<blinding> *d) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  const DeviceWords dd = detail_batch::upload_blinding(d, B);
  DeviceWords dproofs((size_t)9 * B * Context::enc_words());
  std::vector<int> empty((size_t)9 * B, 0);
  rs_rinocchio_pk k{pk.s_pows_.get(), pk.alpha_s_pows_.get(), pk.beta_prods_.get(), pk.beta_rv_ts_.get(),
                    pk.beta_rw_ts_.get(), pk.beta_ry_ts_.get(), 0, 0};
  check(rs_rinocchio_prove_batch(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(), d ? dd.get() : nullptr,
                                 dproofs.get(), empty.data(), nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
inline std::vector<proof> prove_batch(const seeded_proving_key &pk, const std::vector<batch_input> &inputs, const std::vector<blinding> *d) {
  const detail::BatchAssignments a(pk.cs, inputs);
  const int B = a.size();
  const DeviceWords dd = detail_batch::upload_blinding(d, B);
  DeviceWords dproofs((size_t)9 * B * Context::enc_words());
  std::vector<int> empty((size_t)9 * B, 0);
  rs_rinocchio_pk_seeded k{};
  k.s_pows = pk.s_pows_.get(), k.alpha_s_pows = pk.alpha_s_pows_.get(), k.beta_prods = pk.beta_prods_.get();
  std::copy(pk.pub_seeds, pk.pub_seeds + 3, k.pub_seeds);
  k.d_beta_rv_ts = pk.beta_rv_ts_.get(), k.d_beta_rw_ts = pk.beta_rw_ts_.get(), k.d_beta_ry_ts = pk.beta_ry_ts_.get();
  check(rs_rinocchio_prove_batch_seeded(Context::get_context(), pk.cs.get(), &k, B, a.ptrs.data(), a.kinds.data(),
                                        d ? dd.get() : nullptr, dproofs.get(), empty.data(), nullptr));
  return detail_batch::take_proofs(dproofs, empty, B);
}
// as prover(pk, primary, auxiliary): blinding elements sampled per member when the system has auxiliary inputs
template <class PK>
std::vector<proof> prove_batch(const PK &pk, const std::vector<batch_input> &inputs) {
  if (pk.cs.n_vars == pk.cs.n_inputs) return prove_batch(pk, inputs, nullptr);
  const std::vector<blinding> d = detail_batch::sample_blinding(inputs.size());
  return prove_batch(pk, inputs, &d);
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
