// r1cs_solve.hpp -- header-only C++ adapter of the device assignment solver (r1cs_solve.h) on the types of ring.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
#ifndef RINGSNARK_AMD_R1CS_SOLVE_HPP
#define RINGSNARK_AMD_R1CS_SOLVE_HPP

#include <string>

#include "r1cs_solve.h"
#include "ring.hpp"

namespace ringsnark::amd {

// The schedule that completes a full assignment (primary then auxiliary, as is_satisfied and the provers take it) of a
// system already on the device from the wires marked in `given` (one flag per variable, 0-based; the constant one is not a
// variable).  What the reference does with pb.val(...) assignments in gadget order
// (benchmarks/bench_logistic_regression_inference.cpp:147-205), for every wire that is determined through the c side of a
// constraint.  A plan with unsolved wires is still a plan: info() says what is missing and why.  `cs` must outlive it.
class solve_plan {
 public:
  solve_plan(const DeviceR1cs &cs, const std::vector<bool> &given) : n_vars_(cs.n_vars) {
    if (given.size() != cs.n_vars) throw std::invalid_argument("given mask does not match the constraint system");
    const std::vector<uint8_t> mask(given.begin(), given.end());
    check(rs_r1cs_solve_plan_create(Context::get_context(), cs.get(), mask.data(), &h_, &info_));
  }
  ~solve_plan() { rs_r1cs_solve_plan_destroy(h_); }
  solve_plan(const solve_plan &) = delete;
  solve_plan &operator=(const solve_plan &) = delete;
  const rs_r1cs_solve_info &info() const { return info_; }
  rs_r1cs_solve_plan *get() const { return h_; }
  size_t n_vars() const { return n_vars_; }
  // the 0-based variables the plan determines, in the order it determines them
  std::vector<uint32_t> solved_wires() const {
    std::vector<uint32_t> w(info_.n_solved);
    check(rs_r1cs_solve_plan_steps(h_, nullptr, w.data(), nullptr));
    return w;
  }

 private:
  rs_r1cs_solve_plan *h_ = nullptr;
  rs_r1cs_solve_info info_{};
  size_t n_vars_;
};

// Replaces the solved wires of full_assignment by their values; the given wires are read, every other element is neither
// read nor changed (it may be a default-constructed RingElem).  One upload, the solve, one download.  Throws
// std::invalid_argument when the plan leaves wires unsolved, unless allow_partial.
inline rs_r1cs_solve_stats solve(const solve_plan &plan, std::vector<RingElem> &full_assignment, int mode = RS_SOLVE_AUTO,
                                 bool allow_partial = false) {
  if (full_assignment.size() != plan.n_vars()) throw std::invalid_argument("assignment does not match the constraint system");
  const rs_r1cs_solve_info &i = plan.info();
  if (i.n_unsolved && !allow_partial)
    throw std::invalid_argument("the given wires do not determine the assignment: first unsolved variable " + std::to_string(i.first_unsolved) +
                                ", first blocked constraint " + std::to_string(i.first_blocked) + ", reason " + std::to_string(i.blocked_reason));
  std::vector<uint64_t> asg = flatten(full_assignment);
  DeviceWords dasg(asg.data(), asg.size());
  rs_r1cs_solve_stats stats{};
  check(rs_r1cs_solve(Context::get_context(), plan.get(), dasg.get(), mode, &stats, nullptr));
  dasg.download(asg.data());
  const size_t rw = Context::ring_words();
  for (const uint32_t w : plan.solved_wires())
    full_assignment[w] = RingElem(std::vector<uint64_t>(asg.begin() + (size_t)w * rw, asg.begin() + (size_t)(w + 1) * rw));
  return stats;
}

}  // namespace ringsnark::amd
#endif
