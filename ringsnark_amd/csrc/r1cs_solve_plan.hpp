// r1cs_solve_plan.hpp -- the solve plan (include/ringsnark_amd/r1cs_solve.h) as r1cs_solve.hip builds it and as
// r1cs_solve.hip, r1cs_batch.hip and r1cs_hints.hip run it; the scheduler, which r1cs_hints.hip calls with its hints
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/ringsnark_amd/r1cs_solve.h"
#include "../../include/ringsnark_amd/solve_hints.h"

namespace rs {

// one kernel launch of a solve: kind 0 = the level kernel on the constraint steps of one level, 1 = the walk kernel on a run
// of levels, 2 (hint plans only) = the hint-level kernel on the hint steps of one level
struct SolveLaunch {
  int kind;
  size_t s_lo, s_hi;
  double bytes, ops;  // ProfScope: algorithmic bytes and FP64 instructions per lane
};

// what the scheduler adds for a plan with hints (solve_hints.h)
struct HintSchedule {
  std::vector<uint8_t> kinds;  // [n_steps] 0 = constraint step, 1 = hint step
  uint64_t n_wires = 0;        // wires the steps determine
  uint64_t n_run = 0, n_blocked = 0, first_blocked = 0;
};

}  // namespace rs

struct rs_r1cs_solve_plan {
  rs_ctx *ctx = nullptr;
  const rs_r1cs *cs = nullptr;
  rs_r1cs_solve_info info{};
  std::vector<uint32_t> rows, wires;  // the steps, ordered by (level, constraint); of a hint step: the hint and its first target
  std::vector<uint64_t> level_ptr;    // [n_levels + 1]
  std::vector<rs::SolveLaunch> launches[3];  // by mode
  uint32_t *d_rows = nullptr, *d_wires = nullptr;
  uint64_t *d_kinv = nullptr;  // [L][n_steps] constants of the context's arithmetic
};

namespace rs {

// r1cs_solve.hip.  The schedule of r1cs_solve.h into P (info, rows, wires, level_ptr); k: the coefficient sum of every step,
// [n_steps][L] canonical (1 for a hint step).  hints == nullptr: no hints, hs is not touched.  Otherwise the rules of
// solve_hints.h on hints that the caller has VALIDATED, and hs is filled.
void build_schedule(const rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given, rs_r1cs_solve_plan *P, std::vector<uint64_t> &k,
                    const rs_solve_hint *hints = nullptr, size_t n_hints = 0, HintSchedule *hs = nullptr);
// r1cs_solve.hip.  Checks everything of P that indexes memory on the device and uploads d_rows, d_wires and d_kinv.
// n_index: the bound of rows[s] for a hint step (kinds[s] != 0); kinds == nullptr: constraint steps only.
void upload_schedule(const rs_ctx *ctx, rs_r1cs_solve_plan *P, const std::vector<uint64_t> &k, const uint8_t *kinds = nullptr,
                     size_t n_index = 0);
// r1cs_solve.hip.  The launches of kind 0 and 1 on constraint steps only, as rs_r1cs_solve issues them.
void solve_launch(rs_ctx *ctx, const rs_r1cs_solve_plan *P, uint64_t *d_asg, const SolveLaunch &ln, hipStream_t st);
// r1cs_solve.hip.  ln.bytes and ln.ops of a launch on constraint steps; seen: n_vars + 1 words, token: unique per call
void launch_cost(const rs_ctx *ctx, const rs_r1cs_solve_plan *P, std::vector<uint32_t> &seen, uint32_t token, SolveLaunch &ln);

}  // namespace rs
