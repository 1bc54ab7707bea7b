// modswitch.hpp -- header-only C++ adapter of mod-switched encodings and proofs (modswitch.h) on the types of ring.hpp and
// verify.hpp.  A header of its own, as seeded.hpp is; it includes verify.hpp, so one include gives all three.
//
// EncodingElem::modswitch_inplace (ringsnark/seal/seal_ring.hpp:370, seal_ring.tcc:317-322) drops the last prime of each of
// an element's L ciphertexts.  An EncodingElem of ring.hpp always has the context's K primes, so a switched element is a
// type of its own that carries its level -- the number of primes it still has -- and a switched proof is the proof struct
// of the scheme on that type.  The prover switches (no secret involved), the wire carries K_out / K of the words, and
// verifier(vk, primary_input, switched_proof) decodes at the proof's level.
#ifndef RINGSNARK_AMD_MODSWITCH_HPP
#define RINGSNARK_AMD_MODSWITCH_HPP

#include "modswitch.h"
#include "verify.hpp"

namespace ringsnark::amd {

class SwitchedEncodingElem {
 public:
  SwitchedEncodingElem() = default;  // EMPTY (seal_ring.hpp:243,249), at any level
  SwitchedEncodingElem(int level, std::vector<uint64_t> words) : level_(level), w_(std::move(words)) {
    if (level < 1 || level > Context::get_params().K) throw std::invalid_argument("level out of range");
    if (w_.size() != level_words(level)) throw std::invalid_argument("wrong ciphertext size");
  }
  // words of one element of `level` primes: [L][2][level][N_enc]
  static size_t level_words(int level) { return (size_t)Context::get_params().L * 2 * level * Context::get_params().N_enc; }
  bool is_empty() const { return w_.empty(); }
  int level() const { return level_; }
  const std::vector<uint64_t> &words() const { return w_; }
  size_t size_in_bits() const {
    if (w_.empty()) return 0;
    const Params &p = Context::get_params();
    size_t s = 0;
    for (int j = 0; j < level_; j++) s += (size_t)p.L * 2 * p.N_enc * (64 - __builtin_clzll(p.Q[j]));
    return s;
  }
  // EncodingElem::decode at the element's level: the ring element the unswitched encoding holds.  Throws decoding_error
  // when the level was too low for the noise (seal_ring.tcc:446-454).
  static RingElem decode(const EncodingElem::SecretKey &sk, const SwitchedEncodingElem &e) {
    if (e.is_empty()) throw std::invalid_argument("cannot decode an empty encoding");
    const DeviceWords dsk = upload_words(sk), denc = upload_words(e.w_);
    DeviceWords dring(Context::ring_words());
    check(rs_enc_decode_level(Context::get_context(), e.level_, dsk.get(), denc.get(), 1, dring.get(), nullptr));
    std::vector<uint64_t> w(Context::ring_words());
    dring.download(w.data());
    return RingElem(std::move(w));
  }

 private:
  int level_ = 0;
  std::vector<uint64_t> w_;
};

namespace detail {
// the non-EMPTY elements of `in` switched to K_out primes in one call; EMPTY ones stay EMPTY
template <size_t NE>
inline void switch_elems(const EncodingElem *const (&in)[NE], SwitchedEncodingElem *const (&out)[NE], int K_out) {
  const int K = Context::get_params().K;
  if (K_out < 1 || K_out > K) throw std::invalid_argument("level out of range");
  const size_t ew = Context::enc_words(), sw = SwitchedEncodingElem::level_words(K_out);
  std::vector<uint64_t> w;
  size_t n = 0;
  for (size_t k = 0; k < NE; k++)
    if (!in[k]->is_empty()) w.insert(w.end(), in[k]->words().begin(), in[k]->words().end()), n++;
  for (size_t k = 0; k < NE; k++) *out[k] = SwitchedEncodingElem();
  if (n == 0) return;
  const DeviceWords din(w.data(), n * ew);
  DeviceWords dout(n * sw);
  check(rs_enc_mod_switch(Context::get_context(), din.get(), n, K, K_out, dout.get(), nullptr));
  check(rs_sync(Context::get_context(), nullptr));
  std::vector<uint64_t> r(n * sw);
  dout.download(r.data());
  size_t at = 0;
  for (size_t k = 0; k < NE; k++)
    if (!in[k]->is_empty()) {
      *out[k] = SwitchedEncodingElem(K_out, std::vector<uint64_t>(r.begin() + at * sw, r.begin() + (at + 1) * sw));
      at++;
    }
}
// as upload_proof of verify.hpp, on switched elements of one level
template <size_t NE>
inline DeviceWords upload_switched_proof(const SwitchedEncodingElem *const (&elems)[NE], int level, int (&empty)[NE]) {
  const size_t sw = SwitchedEncodingElem::level_words(level);
  std::vector<uint64_t> w(NE * sw, 0);
  for (size_t k = 0; k < NE; k++) {
    empty[k] = elems[k]->is_empty() ? 1 : 0;
    if (empty[k]) continue;
    if (elems[k]->level() != level) throw std::invalid_argument("proof elements of different levels");
    std::memcpy(&w[k * sw], elems[k]->words().data(), sw * 8);
  }
  return DeviceWords(w.data(), w.size());
}
}  // namespace detail

// one element (EncodingElem::modswitch_inplace, K - K_out times)
inline SwitchedEncodingElem mod_switch(const EncodingElem &e, int K_out) {
  SwitchedEncodingElem out;
  const EncodingElem *const in[1] = {&e};
  SwitchedEncodingElem *const o[1] = {&out};
  detail::switch_elems(in, o, K_out);
  return out;
}

namespace groth16 {
struct switched_proof {
  int level = 0;
  SwitchedEncodingElem A, B, C;
  size_t size_in_bits() const { return A.size_in_bits() + B.size_in_bits() + C.size_in_bits(); }
};
inline switched_proof mod_switch(const proof &proof, int K_out) {
  switched_proof out;
  out.level = K_out;
  const EncodingElem *const in[3] = {&proof.A, &proof.B, &proof.C};
  SwitchedEncodingElem *const o[3] = {&out.A, &out.B, &out.C};
  detail::switch_elems(in, o, K_out);
  return out;
}
// groth16::verifier on a switched proof: as verifier(vk, primary_input, proof) of verify.hpp; decoding_error when the level
// was too low for the proof's noise
inline bool verifier(const verification_key_device &vk, const std::vector<RingElem> &primary_input, const switched_proof &proof,
                     rs_verify_report *report = nullptr) {
  if (primary_input.size() != vk.n_inputs) throw std::invalid_argument("primary input does not match the constraint system");
  const SwitchedEncodingElem *const elems[3] = {&proof.A, &proof.B, &proof.C};
  int empty[3];
  const DeviceWords dproof = detail::upload_switched_proof(elems, proof.level, empty), dprimary = detail::upload_primary(primary_input);
  rs_verify_report rep;
  check(rs_groth16_verify_level(Context::get_context(), vk.get(), proof.level, dprimary.get(), dproof.get(), empty, &rep, nullptr));
  if (report) *report = rep;
  return rep.accepted != 0;
}
inline bool verifier(const verification_key &vk, const std::vector<RingElem> &primary_input, const switched_proof &proof) {
  return verifier(verification_key_device(vk), primary_input, proof);
}
}  // namespace groth16

namespace rinocchio {
struct switched_proof {
  int level = 0;
  SwitchedEncodingElem A, A_prime, B, B_prime, C, C_prime, D, D_prime, F;
  size_t size_in_bits() const {
    return A.size_in_bits() + A_prime.size_in_bits() + B.size_in_bits() + B_prime.size_in_bits() + C.size_in_bits() +
           C_prime.size_in_bits() + D.size_in_bits() + D_prime.size_in_bits() + F.size_in_bits();
  }
};
inline switched_proof mod_switch(const proof &proof, int K_out) {
  switched_proof out;
  out.level = K_out;
  const EncodingElem *const in[9] = {&proof.A, &proof.A_prime, &proof.B, &proof.B_prime, &proof.C,
                                     &proof.C_prime, &proof.D, &proof.D_prime, &proof.F};
  SwitchedEncodingElem *const o[9] = {&out.A, &out.A_prime, &out.B, &out.B_prime, &out.C, &out.C_prime, &out.D, &out.D_prime, &out.F};
  detail::switch_elems(in, o, K_out);
  return out;
}
inline bool verifier(const verification_key_device &vk, const std::vector<RingElem> &primary_input, const switched_proof &proof,
                     rs_verify_report *report = nullptr) {
  if (primary_input.size() != vk.n_inputs) throw std::invalid_argument("primary input does not match the constraint system");
  const SwitchedEncodingElem *const elems[9] = {&proof.A, &proof.A_prime, &proof.B, &proof.B_prime, &proof.C,
                                                &proof.C_prime, &proof.D, &proof.D_prime, &proof.F};
  int empty[9];
  const DeviceWords dproof = detail::upload_switched_proof(elems, proof.level, empty), dprimary = detail::upload_primary(primary_input);
  rs_verify_report rep;
  check(rs_rinocchio_verify_level(Context::get_context(), vk.get(), proof.level, dprimary.get(), dproof.get(), empty, &rep, nullptr));
  if (report) *report = rep;
  return rep.accepted != 0;
}
inline bool verifier(const verification_key &vk, const std::vector<RingElem> &primary_input, const switched_proof &proof) {
  return verifier(verification_key_device(vk), primary_input, proof);
}
}  // namespace rinocchio

}  // namespace ringsnark::amd
#endif
