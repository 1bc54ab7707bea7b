// r1cs_batch.hip -- the assignment solver and the satisfaction check for a BATCH of assignments of one system
// (include/ringsnark_amd/r1cs_batch.h): the kernels of r1cs_solve.hip and r1cs_check.hip with one more dimension inside the
// thread.  The members of a batch are independent problems on one schedule and one set of matrices, so a thread owns one slot
// pair of EVERY member: each schedule word, row bound, column index, coefficient and polynomial-table word is loaded once for
// all members, and the thread has one 16-byte assignment load per member in flight where the single kernels have one -- the
// dependent chain (own store -> next load -> arithmetic -> store) that bounds solve_walk_kernel is as long as before and
// carries up to eight times the work.
//
// The member base pointers travel BY VALUE in a kernel-argument struct (BatchAsg): no pointer table in device memory, no
// index computed from assignment data.  Kernels are instantiated for BMAX in {2, 4, 8} slots; the member loops are fully
// unrolled, so the pointer array is only ever indexed by constants and stays in scalar registers, and a slot b >= nb (nb: the
// members of this launch, a kernel argument and therefore wave-uniform) is skipped by a scalar branch: it issues no load, no
// store and no arithmetic.
// The arithmetic is exact and every stored word canonical, so the outputs equal the single kernels' word for word; the sums
// are nevertheless taken in the order of eval_row_pair_skip / solve_step.
#include <algorithm>

#include "../../include/ringsnark_amd/r1cs_batch.h"
#include "r1cs_solve_plan.hpp"
#include "witness_eval.hpp"

namespace rs {

// as r1cs_solve.hip (the AUTO rule is in the plan's launch lists, which are used as they are)
constexpr size_t BATCH_STEPS_PER_WG = 8;
// device side of the reports, the words of r1cs_check.hip per member: [b] key of member b's first violation (all ones: none),
// for b < RS_MAX_BATCH, so that one memset initialises them; then per member REPORT_REST words: violated rows, a, b, c there
constexpr int REPORT_REST = 4;
constexpr int REPORT_WORDS = RS_MAX_BATCH * (1 + REPORT_REST);

// the members' assignments; P is uint64_t * for the solver (neither const nor restrict, for the reason given at
// solve_walk_kernel) and const uint64_t * for the check
template <class P, int BMAX>
struct BatchAsg {
  P p[BMAX];
};

// the three matrices as the kernels read them (SolveCsr of r1cs_solve.hip)
template <class T>
struct BatchCsr {
  const uint32_t *rp[3], *col[3];
  const T *cf[3];  // [L][nnz]
  size_t nnz[3];
  const int32_t *px[3];
  const T *ptab;
};

// bounds of the three rows of one step, its target and k^-1: everything of a step that does not depend on the assignment
template <class T>
struct BatchStep {
  uint32_t e0[3], e1[3], wire;
  T kinv;
};
template <class T>
__device__ __forceinline__ BatchStep<T> load_batch_step(const BatchCsr<T> &cs, const uint32_t *__restrict__ step_row,
                                                        const uint32_t *__restrict__ step_wire, const T *__restrict__ kinv_limb, size_t s) {
  BatchStep<T> st;
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

// eval_row_pair_skip (witness_eval.hpp) for the slot pair of every member: per entry ONE col load, ONE coefficient load and
// ONE pidx / ptab pair load, then a 16-byte assignment load and a multiply-add per member.  Same sums in the same order per
// member, the reduce after every fourth kept term included.  It loads the rows of the terms it keeps and no other, of the
// members b < nb and no other.
template <class M, class P, int BMAX>
__device__ __forceinline__ void eval_row_pair_skip_batch(const uint32_t *__restrict__ col, const typename ArithOf<M>::T *__restrict__ coeff_limb,
                                                         uint32_t e0, uint32_t e1, const BatchAsg<P, BMAX> &asg, int nb, size_t Si, size_t pair,
                                                         uint32_t skip, const M mod, typename ArithOf<M>::T (&o0)[BMAX],
                                                         typename ArithOf<M>::T (&o1)[BMAX], const int32_t *__restrict__ pidx,
                                                         const typename ArithOf<M>::T *__restrict__ ptab) {
  using T = typename ArithOf<M>::T;
  T a0[BMAX], a1[BMAX];
#pragma unroll
  for (int b = 0; b < BMAX; b++) a0[b] = a1[b] = T(0);
  int since = 0;
  for (uint32_t e = e0; e < e1; e++) {
    const uint32_t cv = col[e];
    if (cv == skip) continue;
    T cf0 = coeff_limb[e], cf1 = cf0;  // table constants
    if (pidx) {
      const int32_t pk = pidx[e];
      if (pk >= 0) {
        const T *pc = ptab + (size_t)pk * Si + 2 * pair;
        cf0 = pc[0];
        cf1 = pc[1];
      }
    }
    if (cv == 0) {
      const T k0 = konst_value(cf0, mod), k1 = konst_value(cf1, mod);
#pragma unroll
      for (int b = 0; b < BMAX; b++)
        if (b < nb) {
          a0[b] = addm(a0[b], k0, mod);
          a1[b] = addm(a1[b], k1, mod);
        }
    } else {
      const size_t at = (size_t)(cv - 1) * Si + 2 * pair;  // the same word offset in every member
      ulonglong2 v[BMAX];
#pragma unroll
      for (int b = 0; b < BMAX; b++)
        if (b < nb) v[b] = *reinterpret_cast<const ulonglong2 *>(asg.p[b] + at);
#pragma unroll
      for (int b = 0; b < BMAX; b++)
        if (b < nb) {
          a0[b] = addm(a0[b], mulmod(from_res<T>(v[b].x), cf0, mod), mod);
          a1[b] = addm(a1[b], mulmod(from_res<T>(v[b].y), cf1, mod), mod);
        }
    }
    if (++since == 4) {
      since = 0;
#pragma unroll
      for (int b = 0; b < BMAX; b++)
        if (b < nb) {
          a0[b] = reduce(a0[b], mod);
          a1[b] = reduce(a1[b], mod);
        }
    }
  }
#pragma unroll
  for (int b = 0; b < BMAX; b++)
    if (b < nb) {
      o0[b] = canon(a0[b], mod);
      o1[b] = canon(a1[b], mod);
    }
}

// solve_step of r1cs_solve.hip for every member: target = (<a,z> * <b,z> - <c,z> without the target) * k^-1, canonical
template <class M, int BMAX>
__device__ __forceinline__ void solve_step_batch(const BatchCsr<typename ArithOf<M>::T> &cs, const BatchStep<typename ArithOf<M>::T> &st,
                                                 const BatchAsg<uint64_t *, BMAX> &asg, int nb, size_t S, size_t pair, int limb, const M mod) {
  using T = typename ArithOf<M>::T;
  T x0[BMAX], x1[BMAX], y0[BMAX], y1[BMAX];
  eval_row_pair_skip_batch<M>(cs.col[0], cs.cf[0] + (size_t)limb * cs.nnz[0], st.e0[0], st.e1[0], asg, nb, S, pair, ~0u, mod, x0, x1, cs.px[0], cs.ptab);
  eval_row_pair_skip_batch<M>(cs.col[1], cs.cf[1] + (size_t)limb * cs.nnz[1], st.e0[1], st.e1[1], asg, nb, S, pair, ~0u, mod, y0, y1, cs.px[1], cs.ptab);
  // two canonical residues, one operand centred (the dyadic product of rs_core.hip): the product takes the place of <a,z>
#pragma unroll
  for (int b = 0; b < BMAX; b++)
    if (b < nb) {
      x0[b] = mulmod_dd(x0[b], center(y0[b], mod), mod);
      x1[b] = mulmod_dd(x1[b], center(y1[b], mod), mod);
    }
  eval_row_pair_skip_batch<M>(cs.col[2], cs.cf[2] + (size_t)limb * cs.nnz[2], st.e0[2], st.e1[2], asg, nb, S, pair, st.wire + 1, mod, y0, y1, cs.px[2], cs.ptab);
  const size_t at = (size_t)st.wire * S + 2 * pair;
#pragma unroll
  for (int b = 0; b < BMAX; b++)
    if (b < nb) {
      // the difference is reduced before it meets the constant, per member as in solve_step: |product| <= 0.75 p and c < p
      // leave 1.75 p, beyond what mulmod takes beside |k^-1| <= p / 2 at 50 bits
      const T d0 = reduce(subm(x0[b], y0[b], mod), mod);
      const T d1 = reduce(subm(x1[b], y1[b], mod), mod);
      ulonglong2 o;
      o.x = to_res(canon(mulmod(d0, st.kinv, mod), mod));
      o.y = to_res(canon(mulmod(d1, st.kinv, mod), mod));
      *reinterpret_cast<ulonglong2 *>(asg.p[b] + at) = o;
    }
}

// solve_level_kernel of r1cs_solve.hip with a thread's slot pair of every member.  grid: (slot chunks of 256 slot pairs) x
// (groups of `spw` steps of the level [s_lo, s_hi)), one dimension, ordered by xcd_position.  The rows read (levels below) and
// the rows written (this level) are disjoint in every member, and the members are disjoint (checked on the host).
template <class M, int BMAX>
__global__ void __launch_bounds__(256)
solve_level_batch_kernel(const BatchCsr<typename ArithOf<M>::T> cs, const uint32_t *__restrict__ step_row,
                         const uint32_t *__restrict__ step_wire, const typename ArithOf<M>::T *__restrict__ kinv /* [L][n_steps] */,
                         size_t n_steps, size_t s_lo, size_t s_hi, const BatchAsg<uint64_t *, BMAX> asg, int nb, int N, int L,
                         const M *__restrict__ qmod, unsigned n_groups, unsigned spw) {
  const unsigned pos = xcd_position(blockIdx.x, gridDim.x);
  const unsigned chunk = pos / n_groups, group = pos % n_groups;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)chunk * 256 + threadIdx.x;
  if (2 * pair >= S) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const size_t lo = s_lo + (size_t)group * spw, hi = lo + spw < s_hi ? lo + spw : s_hi;
  for (size_t s = lo; s < hi; s++)
    solve_step_batch<M, BMAX>(cs, load_batch_step(cs, step_row, step_wire, kinv + (size_t)limb * n_steps, s), asg, nb, S, pair, limb, mod);
}

// solve_walk_kernel of r1cs_solve.hip with a thread's slot pair of every member.  grid: slot chunks.  Every thread walks the
// steps [s_lo, s_hi) in order; what a step reads in member b was given or was stored by this very thread in an earlier step,
// so program order is all the ordering there is -- the member pointers are neither const nor restrict, and their loads are
// ordinary vector loads behind the thread's own stores.  The wave-uniform words of step s + 1 are loaded while step s computes.
template <class M, int BMAX>
__global__ void __launch_bounds__(256)
solve_walk_batch_kernel(const BatchCsr<typename ArithOf<M>::T> cs, const uint32_t *__restrict__ step_row,
                        const uint32_t *__restrict__ step_wire, const typename ArithOf<M>::T *__restrict__ kinv /* [L][n_steps] */,
                        size_t n_steps, size_t s_lo, size_t s_hi, const BatchAsg<uint64_t *, BMAX> asg, int nb, int N, int L,
                        const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (2 * pair >= S || s_lo >= s_hi) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const T *kinv_limb = kinv + (size_t)limb * n_steps;
  BatchStep<T> next = load_batch_step(cs, step_row, step_wire, kinv_limb, s_lo);
  for (size_t s = s_lo; s < s_hi; s++) {
    const BatchStep<T> cur = next;
    if (s + 1 < s_hi) next = load_batch_step(cs, step_row, step_wire, kinv_limb, s + 1);
    solve_step_batch<M, BMAX>(cs, cur, asg, nb, S, pair, limb, mod);
  }
}

// one row of the check for the members [0, nb) of `asg`: keys at rep[b], flag rows at flags + b * m
template <class M, int G>
__device__ __forceinline__ void check_row_batch(const BatchCsr<typename ArithOf<M>::T> &cs, const BatchAsg<const uint64_t *, G> &asg, int nb,
                                                size_t row, size_t m, size_t S, size_t pair, int limb, const M mod, uint8_t *__restrict__ flags,
                                                unsigned long long *__restrict__ rep) {
  using T = typename ArithOf<M>::T;
  T x0[G], x1[G], y0[G], y1[G];
  eval_row_pair_skip_batch<M>(cs.col[0], cs.cf[0] + (size_t)limb * cs.nnz[0], cs.rp[0][row], cs.rp[0][row + 1], asg, nb, S, pair, ~0u, mod, x0, x1, cs.px[0], cs.ptab);
  eval_row_pair_skip_batch<M>(cs.col[1], cs.cf[1] + (size_t)limb * cs.nnz[1], cs.rp[1][row], cs.rp[1][row + 1], asg, nb, S, pair, ~0u, mod, y0, y1, cs.px[1], cs.ptab);
  // two canonical residues: one operand centred, as the dyadic product of rs_core.hip
#pragma unroll
  for (int b = 0; b < G; b++)
    if (b < nb) {
      x0[b] = canon(mulmod_dd(x0[b], center(y0[b], mod), mod), mod);
      x1[b] = canon(mulmod_dd(x1[b], center(y1[b], mod), mod), mod);
    }
  eval_row_pair_skip_batch<M>(cs.col[2], cs.cf[2] + (size_t)limb * cs.nnz[2], cs.rp[2][row], cs.rp[2][row + 1], asg, nb, S, pair, ~0u, mod, y0, y1, cs.px[2], cs.ptab);
#pragma unroll
  for (int b = 0; b < G; b++)
    if (b < nb) {
      const bool bad0 = x0[b] != y0[b], bad1 = x1[b] != y1[b];
      const unsigned long long bad = __ballot(bad0 || bad1);
      if (bad == 0ull) continue;  // wave-uniform: the common path ends here
      // the lanes of a wave hold one row and ascending slot pairs: the lowest violating lane has the wave's smallest key
      if ((int)(threadIdx.x & 63u) == __ffsll(bad) - 1) {
        flags[(size_t)b * m + row] = 1;
        atomicMin(rep + b, (unsigned long long)(row * S + 2 * pair + (bad0 ? 0 : 1)));
      }
    }
}

// members one pass over a row carries in the check kernel: all BMAX slots, except eight slots of the integer arithmetic,
// which the compiler gives 256 VGPRs and 20 AGPRs (one wave per SIMD) and which go in two passes of four instead (139 VGPRs,
// three waves); the second pass finds the row's matrix words in L1.  profiles/r1cs_batch_resources.txt has every kernel.
template <class M, int BMAX>
constexpr int check_pass_slots() {
  return (std::is_same<M, ModI>::value && BMAX == 8) ? 4 : BMAX;
}

// r1cs_check_kernel of r1cs_check.hip with a thread's slot pair of every member: grid (slot chunks of 256 slot pairs) x (row
// groups of `rpw` rows), one dimension, ordered by xcd_position.  One row at a time (the rows-in-flight factor of the single
// kernel, CHECK_R = 2, bought two independent load chains per lane; the members give up to eight).  Member b has its own key
// word rep[b] and its own flag row flags + b * m, written by the scheme of the single kernel: the lowest violating lane of a
// wave stores the flag byte and takes the 64-bit atomicMin, so every field is a function of member b's inputs only.
template <class M, int BMAX>
__global__ void __launch_bounds__(256)
r1cs_check_batch_kernel(const BatchCsr<typename ArithOf<M>::T> cs, const BatchAsg<const uint64_t *, BMAX> asg, int nb, size_t m, int N, int L,
                        const M *__restrict__ qmod, unsigned n_groups, unsigned rpw, uint8_t *__restrict__ flags,
                        unsigned long long *__restrict__ rep) {
  constexpr int G = check_pass_slots<M, BMAX>();
  const unsigned pos = xcd_position(blockIdx.x, gridDim.x);
  const unsigned chunk = pos / n_groups, group = pos % n_groups;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)chunk * 256 + threadIdx.x;
  if (2 * pair >= S) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const size_t row_lo = (size_t)group * rpw, row_hi = row_lo + rpw < m ? row_lo + rpw : m;
  for (size_t row = row_lo; row < row_hi; row++) {
#pragma unroll
    for (int g0 = 0; g0 < BMAX; g0 += G) {
      if (g0 >= nb) break;  // wave-uniform
      BatchAsg<const uint64_t *, G> part;
#pragma unroll
      for (int b = 0; b < G; b++) part.p[b] = asg.p[g0 + b];
      check_row_batch<M, G>(cs, part, nb - g0, row, m, S, pair, limb, mod, flags + (size_t)g0 * m, rep + g0);
    }
  }
}

// r1cs_check_finish_kernel of r1cs_check.hip, the member in blockIdx.y: counts member b's flag bytes and evaluates the three
// rows once at its first violation.  The member's pointer is picked by an unrolled compare, not by indexing the argument.
template <class M>
__global__ void __launch_bounds__(256)
r1cs_check_batch_finish_kernel(const BatchCsr<typename ArithOf<M>::T> cs, const BatchAsg<const uint64_t *, RS_MAX_BATCH> members, size_t m,
                               int N, int L, unsigned n_inputs, const M *__restrict__ qmod, const uint8_t *__restrict__ all_flags,
                               unsigned long long *__restrict__ all_rep) {
  using T = typename ArithOf<M>::T;
  __shared__ unsigned wave_count[4];
  const unsigned member = blockIdx.y;
  const uint8_t *flags = all_flags + (size_t)member * m;
  unsigned long long *rep = all_rep + RS_MAX_BATCH + (size_t)member * REPORT_REST;  // violated rows, a, b, c
  unsigned n = 0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x) n += flags[r] ? 1u : 0u;
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if ((threadIdx.x & 63u) == 0) wave_count[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const unsigned total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
  if (total) atomicAdd(rep, (unsigned long long)total);
  const unsigned long long key = all_rep[member];  // final: written by the launch before this one
  if (blockIdx.x != 0 || key == ~0ull) return;
  const uint64_t *asg = members.p[0];
#pragma unroll
  for (int b = 1; b < RS_MAX_BATCH; b++)
    if (member == (unsigned)b) asg = members.p[b];
  const size_t S = (size_t)L * N, row = (size_t)(key / S), idx = (size_t)(key % S), pair = idx >> 1;
  const int limb = (int)(idx / (size_t)N);
  const M mod = qmod[limb];
  T x0, x1;
  eval_row_pair<M>(cs.rp[0], cs.col[0], cs.cf[0] + (size_t)limb * cs.nnz[0], row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, cs.px[0], cs.ptab);
  rep[1] = to_res((idx & 1) ? x1 : x0);
  eval_row_pair<M>(cs.rp[1], cs.col[1], cs.cf[1] + (size_t)limb * cs.nnz[1], row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, cs.px[1], cs.ptab);
  rep[2] = to_res((idx & 1) ? x1 : x0);
  eval_row_pair<M>(cs.rp[2], cs.col[2], cs.cf[2] + (size_t)limb * cs.nnz[2], row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, cs.px[2], cs.ptab);
  rep[3] = to_res((idx & 1) ? x1 : x0);
}

template <class T>
static BatchCsr<T> batch_csr(const rs_r1cs *cs) {
  BatchCsr<T> k;
  for (int w = 0; w < 3; w++) {
    k.rp[w] = cs->d_row_ptr[w];
    k.col[w] = cs->d_col[w];
    k.cf[w] = reinterpret_cast<const T *>(cs->d_coeff[w]);
    k.nnz[w] = cs->nnz[w];
    k.px[w] = cs->d_pidx[w];
  }
  k.ptab = reinterpret_cast<const T *>(cs->d_ptab);
  return k;
}

// the slots of a launch that has no member hold null: the kernels never touch a slot b >= nb
template <class P, int BMAX>
static BatchAsg<P, BMAX> batch_asg(P const *members, int nb) {
  BatchAsg<P, BMAX> a;
  for (int b = 0; b < BMAX; b++) a.p[b] = b < nb ? members[b] : nullptr;
  return a;
}

// run `f` with the smallest instantiated slot count that holds nb members (2 <= nb <= RS_MAX_BATCH) as a compile-time constant
template <class F>
static void dispatch_slots(int nb, F &&f) {
  if (nb <= 2) f(std::integral_constant<int, 2>{});
  else if (nb <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// solve_run of r1cs_solve.hip: the plan's launches, each once for the whole batch
template <class M, int BMAX>
static void solve_batch_run(rs_ctx *ctx, const rs_r1cs_solve_plan *P, uint64_t *const *members, int nb, const std::vector<SolveLaunch> &launches,
                            hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const BatchCsr<T> k = batch_csr<T>(P->cs);
  const BatchAsg<uint64_t *, BMAX> asg = batch_asg<uint64_t *, BMAX>(members, nb);
  const T *kinv = reinterpret_cast<const T *>(P->d_kinv);
  const size_t n_steps = P->rows.size(), chunks = (ctx->ring_words() / 2 + 255) / 256;
  for (const SolveLaunch &ln : launches) {
    if (ln.kind == 0) {
      size_t spw = BATCH_STEPS_PER_WG;
      while (spw > 1 && chunks * ((ln.s_hi - ln.s_lo + spw - 1) / spw) < 4096) spw >>= 1;
      const size_t groups = (ln.s_hi - ln.s_lo + spw - 1) / spw;
      RS_REQUIRE(chunks * groups < ((size_t)1 << 31), "level too wide for one launch of the solver");
      ProfScope p(ctx, st, "solve_level_batch", ln.bytes * nb, ln.ops * nb);
      hipLaunchKernelGGL((solve_level_batch_kernel<M, BMAX>), dim3((unsigned)(chunks * groups)), dim3(256), 0, st, k, P->d_rows, P->d_wires,
                         kinv, n_steps, ln.s_lo, ln.s_hi, asg, nb, ctx->N, ctx->L, CtxArith<M>::qmod(ctx), (unsigned)groups, (unsigned)spw);
    } else {
      ProfScope p(ctx, st, "solve_walk_batch", ln.bytes * nb, ln.ops * nb);
      hipLaunchKernelGGL((solve_walk_batch_kernel<M, BMAX>), dim3((unsigned)chunks), dim3(256), 0, st, k, P->d_rows, P->d_wires, kinv,
                         n_steps, ln.s_lo, ln.s_hi, asg, nb, ctx->N, ctx->L, CtxArith<M>::qmod(ctx));
    }
    RS_HIP(hipGetLastError());
  }
}

template <class M, int BMAX>
static void check_batch_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *const *members, int nb, uint8_t *flags, unsigned long long *rep,
                            hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const size_t S = ctx->ring_words(), m = cs->m;
  const size_t chunks = (S / 2 + 255) / 256;
  // rows per workgroup: the rule of r1cs_check_run, down to one row
  size_t rpw = 16;
  while (rpw > 1 && chunks * ((m + rpw - 1) / rpw) < 4096) rpw >>= 1;
  const size_t groups = (m + rpw - 1) / rpw;
  RS_REQUIRE(chunks * groups < ((size_t)1 << 31), "constraint system too large for one launch of the check");
  const BatchCsr<T> k = batch_csr<T>(cs);
  double nnz = 0;
  for (int w = 0; w < 3; w++) nnz += (double)cs->nnz[w];
  {
    // algorithmic bytes: every member's assignment once and the three CSRs once
    ProfScope p(ctx, st, "r1cs_check_batch", (double)nb * cs->n_vars * S * 8 + nnz * (4 + 8.0 * ctx->L) + 3.0 * (m + 1) * 4,
                7.0 * (nnz + m) * S * nb);
    hipLaunchKernelGGL((r1cs_check_batch_kernel<M, BMAX>), dim3((unsigned)(chunks * groups)), dim3(256), 0, st, k,
                       (batch_asg<const uint64_t *, BMAX>(members, nb)), nb, m, ctx->N, ctx->L, CtxArith<M>::qmod(ctx), (unsigned)groups,
                       (unsigned)rpw, flags, rep);
  }
  RS_HIP(hipGetLastError());
  const unsigned fin_blocks = (unsigned)std::min<size_t>((m + 255) / 256, 64);
  hipLaunchKernelGGL(r1cs_check_batch_finish_kernel<M>, dim3(fin_blocks, (unsigned)nb), dim3(256), 0, st, k,
                     (batch_asg<const uint64_t *, RS_MAX_BATCH>(members, nb)), m, ctx->N, ctx->L, (unsigned)cs->n_inputs, CtxArith<M>::qmod(ctx),
                     flags, rep);
  RS_HIP(hipGetLastError());
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_r1cs_solve_batch(rs_ctx *ctx, const rs_r1cs_solve_plan *plan, int batch, uint64_t *const *d_assignments, int mode,
                        rs_r1cs_solve_stats *h_stats, rs_stream stream) {
  if (ctx && plan && d_assignments && batch == 1) return rs_r1cs_solve(ctx, plan, d_assignments[0], mode, h_stats, stream);
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(plan && d_assignments, "null argument");
  RS_REQUIRE(batch >= 1 && batch <= RS_MAX_BATCH, "batch out of range");
  for (int b = 0; b < batch; b++) RS_REQUIRE(d_assignments[b], "null batch member");
  RS_REQUIRE(plan->ctx == ctx, "solve plan of another context");
  RS_REQUIRE(mode == RS_SOLVE_AUTO || mode == RS_SOLVE_LEVELS || mode == RS_SOLVE_WALK, "unknown solve mode");
  {
    // the members are written: their byte ranges [p, p + n_vars * L * N * 8) must be disjoint
    uintptr_t lo[RS_MAX_BATCH];
    for (int b = 0; b < batch; b++) lo[b] = (uintptr_t)d_assignments[b];
    std::sort(lo, lo + batch);
    const uintptr_t bytes = (uintptr_t)plan->cs->n_vars * ctx->ring_words() * sizeof(uint64_t);
    for (int b = 0; b + 1 < batch; b++) RS_REQUIRE(lo[b + 1] - lo[b] >= bytes, "batch members overlap");
  }
  const std::vector<SolveLaunch> &launches = plan->launches[mode];
  rs_r1cs_solve_stats stats{0, 0};
  for (const SolveLaunch &ln : launches) (ln.kind == 0 ? stats.level_launches : stats.walk_launches)++;
  if (!launches.empty()) {
    std::unique_lock<std::mutex> lk(ctx->mu, std::defer_lock);
    if (ctx->profiling) lk.lock();  // the record ProfScope appends to belongs to the holder of mu
    dispatch_arith(ctx, [&](auto tag) {
      dispatch_slots(batch, [&](auto slots) {
        solve_batch_run<decltype(tag), decltype(slots)::value>(ctx, plan, d_assignments, batch, launches, S(stream));
      });
    });
  }
  if (h_stats) *h_stats = stats;
  RS_API_END
}

int rs_r1cs_check_batch(rs_ctx *ctx, const rs_r1cs *cs, int batch, const uint64_t *const *d_assignments, uint8_t *d_row_flags,
                        rs_r1cs_report *h_reports, rs_stream stream) {
  if (ctx && cs && d_assignments && h_reports && batch == 1) return rs_r1cs_check(ctx, cs, d_assignments[0], d_row_flags, h_reports, stream);
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(cs && d_assignments && h_reports, "null argument");
  RS_REQUIRE(batch >= 1 && batch <= RS_MAX_BATCH, "batch out of range");
  for (int b = 0; b < batch; b++) RS_REQUIRE(d_assignments[b], "null batch member");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  const size_t m = cs->m, words = ctx->ring_words();
  rs_r1cs_report none{};
  none.first_row = m;
  if (m && words) {
    hipStream_t st = S(stream);
    WsScope ws_scope(ctx, st);
    // workspace: the report words, then (unless the caller brought them) the flag rows
    const size_t rep_bytes = sizeof(unsigned long long) * REPORT_WORDS;
    char *ws = (char *)ws_get(ctx, WS_SMALL, std::max<size_t>(256, rep_bytes + (d_row_flags ? 0 : (size_t)batch * m)));
    unsigned long long *rep = (unsigned long long *)ws;
    uint8_t *flags = d_row_flags ? d_row_flags : (uint8_t *)(ws + rep_bytes);
    RS_HIP(hipMemsetAsync(rep, 0, rep_bytes, st));
    RS_HIP(hipMemsetAsync(rep, 0xFF, sizeof(unsigned long long) * RS_MAX_BATCH, st));
    RS_HIP(hipMemsetAsync(flags, 0, (size_t)batch * m, st));
    dispatch_arith(ctx, [&](auto tag) {
      dispatch_slots(batch, [&](auto slots) {
        check_batch_run<decltype(tag), decltype(slots)::value>(ctx, cs, d_assignments, batch, flags, rep, st);
      });
    });
    unsigned long long h[REPORT_WORDS];
    RS_HIP(hipMemcpyAsync(h, rep, rep_bytes, hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < batch; b++) {
      const unsigned long long key = h[b], *hb = h + RS_MAX_BATCH + (size_t)b * REPORT_REST;
      rs_r1cs_report out = none;
      out.n_violated = hb[0];
      if (key != ~0ull) {
        const size_t idx = (size_t)(key % words);
        out.first_row = (uint64_t)(key / words);
        out.first_limb = (uint32_t)(idx / (size_t)ctx->N);
        out.first_slot = (uint32_t)(idx % (size_t)ctx->N);
        out.a = hb[1];
        out.b = hb[2];
        out.c = hb[3];
      }
      h_reports[b] = out;
    }
  } else {
    if (d_row_flags && m) {
      RS_HIP(hipMemsetAsync(d_row_flags, 0, (size_t)batch * m, S(stream)));
      RS_HIP(hipStreamSynchronize(S(stream)));
    }
    for (int b = 0; b < batch; b++) h_reports[b] = none;
  }
  RS_API_END
}

}  // extern "C"
