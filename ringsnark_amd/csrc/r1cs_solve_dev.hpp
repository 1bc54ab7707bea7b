// r1cs_solve_dev.hpp -- the device pieces of the assignment solver that r1cs_solve.hip and r1cs_hints.hip share: the
// matrices as the kernels read them, a step's assignment-independent words, and the step itself
#pragma once
#include "witness_eval.hpp"

namespace rs {

// the three matrices as the kernels read them
template <class T>
struct SolveCsr {
  const uint32_t *rp[3], *col[3];
  const T *cf[3];  // [L][nnz]
  size_t nnz[3];
  const int32_t *px[3];
  const T *ptab;
};

// bounds of the three rows of one step, its target and k^-1: everything of a step that does not depend on the assignment
template <class T>
struct SolveStep {
  uint32_t e0[3], e1[3], wire;
  T kinv;
};
template <class T>
__device__ __forceinline__ SolveStep<T> load_step(const SolveCsr<T> &cs, const uint32_t *__restrict__ step_row,
                                                  const uint32_t *__restrict__ step_wire, const T *__restrict__ kinv_limb, size_t s) {
  SolveStep<T> st;
  const uint32_t row = step_row[s];
#pragma unroll
  for (int w = 0; w < 3; w++) {
    st.e0[w] = cs.rp[w][row];
    st.e1[w] = cs.rp[w][row + 1];
  }
  st.wire = step_wire[s];
  st.kinv = kinv_limb[s];
  return st;
}

// target = (<a,z> * <b,z> - <c,z> without the target) * k^-1 for one slot pair, stored as canonical residues
template <class M>
__device__ __forceinline__ void solve_step(const SolveCsr<typename ArithOf<M>::T> &cs, const SolveStep<typename ArithOf<M>::T> &st,
                                           uint64_t *asg, size_t S, size_t pair, int limb, const M mod) {
  using T = typename ArithOf<M>::T;
  T a0, a1, b0, b1, c0, c1;
  eval_row_pair_skip<M>(cs.col[0], cs.cf[0] + (size_t)limb * cs.nnz[0], st.e0[0], st.e1[0], asg, S, pair, ~0u, mod, a0, a1, cs.px[0], cs.ptab);
  eval_row_pair_skip<M>(cs.col[1], cs.cf[1] + (size_t)limb * cs.nnz[1], st.e0[1], st.e1[1], asg, S, pair, ~0u, mod, b0, b1, cs.px[1], cs.ptab);
  eval_row_pair_skip<M>(cs.col[2], cs.cf[2] + (size_t)limb * cs.nnz[2], st.e0[2], st.e1[2], asg, S, pair, st.wire + 1, mod, c0, c1, cs.px[2], cs.ptab);
  // two canonical residues, one operand centred (the dyadic product of rs_core.hip); the difference is reduced before it
  // meets the constant: |product| <= 0.75 p and c < p leave 1.75 p, beyond what mulmod takes beside |k^-1| <= p / 2 at 50 bits
  const T d0 = reduce(subm(mulmod_dd(a0, center(b0, mod), mod), c0, mod), mod);
  const T d1 = reduce(subm(mulmod_dd(a1, center(b1, mod), mod), c1, mod), mod);
  ulonglong2 o;
  o.x = to_res(canon(mulmod(d0, st.kinv, mod), mod));
  o.y = to_res(canon(mulmod(d1, st.kinv, mod), mod));
  reinterpret_cast<ulonglong2 *>(asg + (size_t)st.wire * S)[pair] = o;
}

}  // namespace rs
