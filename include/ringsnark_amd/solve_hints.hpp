// solve_hints.hpp -- header-only C++ adapter of the device assignment solver with hints (solve_hints.h) on the types of
// ring.hpp.  Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
#ifndef RINGSNARK_AMD_SOLVE_HINTS_HPP
#define RINGSNARK_AMD_SOLVE_HINTS_HPP

#include <string>

#include "ring.hpp"
#include "solve_hints.h"

namespace ringsnark::amd {

// 0-based variables, as the elements of a full assignment
inline rs_solve_hint bits_hint(uint32_t src, uint32_t dst, uint32_t nbits, uint32_t dst_stride = 1) {
  return rs_solve_hint{RS_HINT_BITS, src, 0, dst, nbits, dst_stride};
}
inline rs_solve_hint inv_hint(uint32_t src, uint32_t dst) { return rs_solve_hint{RS_HINT_INV, src, 0, dst, 0, 1}; }
inline rs_solve_hint quot_hint(uint32_t num, uint32_t src, uint32_t dst) { return rs_solve_hint{RS_HINT_QUOT, src, num, dst, 0, 1}; }

// The schedule that completes a full assignment of a system already on the device from the wires marked in `given` and the
// declared hints: solve_plan (r1cs_solve.hpp) with the bit, inverse and quotient wires of wires the solver itself produces.
// A hint the library refuses (solve_hints.h lists them) throws.  A plan with unsolved wires or blocked hints is still a plan:
// info() says what is missing and why.  `cs` must outlive it.
class hint_plan {
 public:
  hint_plan(const DeviceR1cs &cs, const std::vector<bool> &given, const std::vector<rs_solve_hint> &hints) : n_vars_(cs.n_vars), hints_(hints) {
    if (given.size() != cs.n_vars) throw std::invalid_argument("given mask does not match the constraint system");
    const std::vector<uint8_t> mask(given.begin(), given.end());
    check(rs_r1cs_hint_plan_create(Context::get_context(), cs.get(), mask.data(), hints_.data(), hints_.size(), &h_, &info_));
  }
  ~hint_plan() { rs_r1cs_hint_plan_destroy(h_); }
  hint_plan(const hint_plan &) = delete;
  hint_plan &operator=(const hint_plan &) = delete;
  const rs_r1cs_hint_info &info() const { return info_; }
  rs_r1cs_hint_plan *get() const { return h_; }
  size_t n_vars() const { return n_vars_; }
  // the 0-based variables the plan determines, in the order it determines them: the target of a constraint step, every
  // target of a hint step
  std::vector<uint32_t> solved_wires() const {
    std::vector<uint8_t> kind(info_.n_steps);
    std::vector<uint32_t> index(info_.n_steps), wire(info_.n_steps), out;
    check(rs_r1cs_hint_plan_steps(h_, kind.data(), index.data(), wire.data(), nullptr));
    for (size_t s = 0; s < kind.size(); s++) {
      const size_t n = kind[s] && hints_[index[s]].kind == RS_HINT_BITS ? hints_[index[s]].nbits : 1;
      const size_t stride = kind[s] && hints_[index[s]].kind == RS_HINT_BITS ? hints_[index[s]].dst_stride : 1;
      for (size_t t = 0; t < n; t++) out.push_back((uint32_t)(wire[s] + t * stride));
    }
    return out;
  }

 private:
  rs_r1cs_hint_plan *h_ = nullptr;
  rs_r1cs_hint_info info_{};
  size_t n_vars_;
  std::vector<rs_solve_hint> hints_;
};

// Replaces the solved wires of full_assignment by their values; the given wires are read, every other element is neither
// read nor changed (it may be a default-constructed RingElem).  One upload, the solve, one download.  *report says where a
// BITS source does not fit its bits and where an INV or QUOT source is zero: answers, not errors.  Throws
// std::invalid_argument when the plan leaves wires unsolved, unless allow_partial.
inline rs_r1cs_hint_stats solve_hinted(const hint_plan &plan, std::vector<RingElem> &full_assignment, int mode = RS_SOLVE_AUTO,
                                       rs_solve_hint_report *report = nullptr, bool allow_partial = false) {
  if (full_assignment.size() != plan.n_vars()) throw std::invalid_argument("assignment does not match the constraint system");
  const rs_r1cs_hint_info &i = plan.info();
  if (i.solve.n_unsolved && !allow_partial)
    throw std::invalid_argument("the given wires and the hints do not determine the assignment: first unsolved variable " +
                                std::to_string(i.solve.first_unsolved) + ", first blocked constraint " + std::to_string(i.solve.first_blocked) +
                                ", reason " + std::to_string(i.solve.blocked_reason) + ", hints never ready " + std::to_string(i.n_hints_blocked));
  std::vector<uint64_t> asg = flatten(full_assignment);
  DeviceWords dasg(asg.data(), asg.size());
  rs_r1cs_hint_stats stats{};
  rs_solve_hint_report rep{};
  check(rs_r1cs_solve_hinted(Context::get_context(), plan.get(), dasg.get(), mode, &stats, &rep, nullptr));
  if (report) *report = rep;
  dasg.download(asg.data());
  const size_t rw = Context::ring_words();
  for (const uint32_t w : plan.solved_wires())
    full_assignment[w] = RingElem(std::vector<uint64_t>(asg.begin() + (size_t)w * rw, asg.begin() + (size_t)(w + 1) * rw));
  return stats;
}

}  // namespace ringsnark::amd
#endif
