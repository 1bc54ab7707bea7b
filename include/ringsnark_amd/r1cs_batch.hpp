// r1cs_batch.hpp -- header-only C++ adapter of the batched assignment solver and satisfaction check (r1cs_batch.h) on the
// types of ring.hpp, r1cs_solve.hpp and r1cs_check.hpp, which it includes.  Beside ring.hpp for the reason given in
// r1cs_check.h.
#ifndef RINGSNARK_AMD_R1CS_BATCH_HPP
#define RINGSNARK_AMD_R1CS_BATCH_HPP

#include <string>

#include "r1cs_batch.h"
#include "r1cs_check.hpp"
#include "r1cs_solve.hpp"

namespace ringsnark::amd {

namespace detail {
inline std::vector<DeviceWords> upload_members(const std::vector<std::vector<RingElem>> &members, size_t n_vars) {
  if (members.empty() || members.size() > RS_MAX_BATCH) throw std::invalid_argument("a batch holds 1 to " + std::to_string(RS_MAX_BATCH) + " assignments");
  std::vector<DeviceWords> d;
  for (const auto &a : members) {
    if (a.size() != n_vars) throw std::invalid_argument("assignment does not match the constraint system");
    const std::vector<uint64_t> words = flatten(a);
    d.emplace_back(words.data(), words.size());
  }
  return d;
}
}  // namespace detail

// solve (r1cs_solve.hpp) for 1 to RS_MAX_BATCH full assignments of one plan in one pass over the schedule and the system:
// the solved wires of every member are replaced by their values, word for word as solve() computes them; the given wires
// are read, every other element is neither read nor changed.  One upload per member, one solve, one download per member.
// The statistics are those of the whole batch.  Throws std::invalid_argument when the plan leaves wires unsolved, unless
// allow_partial.
inline rs_r1cs_solve_stats solve_batch(const solve_plan &plan, std::vector<std::vector<RingElem>> &full_assignments, int mode = RS_SOLVE_AUTO,
                                       bool allow_partial = false) {
  const rs_r1cs_solve_info &i = plan.info();
  if (i.n_unsolved && !allow_partial)
    throw std::invalid_argument("the given wires do not determine the assignment: first unsolved variable " + std::to_string(i.first_unsolved) +
                                ", first blocked constraint " + std::to_string(i.first_blocked) + ", reason " + std::to_string(i.blocked_reason));
  const std::vector<DeviceWords> d = detail::upload_members(full_assignments, plan.n_vars());
  std::vector<uint64_t *> ptrs;
  for (const auto &w : d) ptrs.push_back(w.get());
  rs_r1cs_solve_stats stats{};
  check(rs_r1cs_solve_batch(Context::get_context(), plan.get(), (int)ptrs.size(), ptrs.data(), mode, &stats, nullptr));
  const size_t rw = Context::ring_words();
  const std::vector<uint32_t> wires = plan.solved_wires();
  std::vector<uint64_t> asg(plan.n_vars() * rw);
  for (size_t b = 0; b < d.size(); b++) {
    d[b].download(asg.data());
    for (const uint32_t w : wires)
      full_assignments[b][w] = RingElem(std::vector<uint64_t>(asg.begin() + (size_t)w * rw, asg.begin() + (size_t)(w + 1) * rw));
  }
  return stats;
}

// is_satisfied (r1cs_check.hpp) for 1 to RS_MAX_BATCH full assignments (primary then auxiliary) of one system in one pass
// over its matrices: one report per member, n_violated == 0 being the reference's `true`.
inline std::vector<r1cs_violation> is_satisfied_batch(const DeviceR1cs &cs, const std::vector<std::vector<RingElem>> &full_assignments) {
  const std::vector<DeviceWords> d = detail::upload_members(full_assignments, cs.n_vars);
  std::vector<const uint64_t *> ptrs;
  for (const auto &w : d) ptrs.push_back(w.get());
  std::vector<rs_r1cs_report> rep(ptrs.size());
  check(rs_r1cs_check_batch(Context::get_context(), cs.get(), (int)ptrs.size(), ptrs.data(), nullptr, rep.data(), nullptr));
  std::vector<r1cs_violation> out;
  for (const rs_r1cs_report &r : rep)
    out.push_back(r1cs_violation{(size_t)r.n_violated, (size_t)r.first_row, (int)r.first_limb, (int)r.first_slot, r.a, r.b, r.c});
  return out;
}

}  // namespace ringsnark::amd
#endif
