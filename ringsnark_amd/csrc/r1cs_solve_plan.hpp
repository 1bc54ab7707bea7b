// r1cs_solve_plan.hpp -- the solve plan (include/ringsnark_amd/r1cs_solve.h) as r1cs_solve.hip builds it and as
// r1cs_solve.hip and r1cs_batch.hip run it
#pragma once
#include <vector>

#include "../../include/ringsnark_amd/r1cs_solve.h"

namespace rs {

// one kernel launch of a solve: kind 0 = the level kernel on one level, 1 = the walk kernel on a run of levels
struct SolveLaunch {
  int kind;
  size_t s_lo, s_hi;
  double bytes, ops;  // ProfScope: algorithmic bytes and FP64 instructions per lane
};

}  // namespace rs

struct rs_r1cs_solve_plan {
  rs_ctx *ctx = nullptr;
  const rs_r1cs *cs = nullptr;
  rs_r1cs_solve_info info{};
  std::vector<uint32_t> rows, wires;  // the steps, ordered by (level, constraint)
  std::vector<uint64_t> level_ptr;    // [n_levels + 1]
  std::vector<rs::SolveLaunch> launches[3];  // by mode
  uint32_t *d_rows = nullptr, *d_wires = nullptr;
  uint64_t *d_kinv = nullptr;  // [L][n_steps] constants of the context's arithmetic
};
