// r1cs_check.hpp -- header-only C++ adapter of the device satisfaction check (r1cs_check.h) on the types of ring.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
#ifndef RINGSNARK_AMD_R1CS_CHECK_HPP
#define RINGSNARK_AMD_R1CS_CHECK_HPP

#include "r1cs_check.h"
#include "ring.hpp"

namespace ringsnark::amd {

// r1cs_constraint_system::is_satisfied (relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:122-158) on a system
// already on the device, with the reference's argument order: what its provers assert before they start
// (r1cs_to_qrp.tcc:156, groth16.tcc:74).  One upload of the assignment, one fused pass (rs_r1cs_check); `where` says which
// constraint fails first, in which limb and slot, and with which three values.
struct r1cs_violation {
  size_t n_violated, constraint;
  int limb, slot;
  uint64_t a, b, c;
};
inline bool is_satisfied(const DeviceR1cs &cs, const std::vector<RingElem> &primary_input,
                         const std::vector<RingElem> &auxiliary_input, r1cs_violation *where = nullptr) {
  if (primary_input.size() != cs.n_inputs || primary_input.size() + auxiliary_input.size() != cs.n_vars)
    throw std::invalid_argument("assignment does not match the constraint system");
  std::vector<RingElem> full(primary_input);
  full.insert(full.end(), auxiliary_input.begin(), auxiliary_input.end());
  const std::vector<uint64_t> asg = flatten(full);
  DeviceWords dasg(asg.data(), asg.size());
  rs_r1cs_report rep;
  check(rs_r1cs_check(Context::get_context(), cs.get(), dasg.get(), nullptr, &rep, nullptr));
  if (where) *where = r1cs_violation{(size_t)rep.n_violated, (size_t)rep.first_row, (int)rep.first_limb, (int)rep.first_slot, rep.a, rep.b, rep.c};
  return rep.n_violated == 0;
}

}  // namespace ringsnark::amd
#endif
