// r1cs_check.hip -- r1cs_constraint_system::is_satisfied (relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:122-158)
// on the device: <a,(1,x)> * <b,(1,x)> == <c,(1,x)> for every constraint, in every slot of every limb, in ONE pass over the
// assignment and without any [m][L][N] intermediate -- plus WHERE it fails.
//
// Every reported field is a function of the inputs only:
//   flags[row]   a plain byte store of 1 by a lane that found a violation (all writers write the same value)
//   first        64-bit atomicMin over the key row * L*N + limb * N + slot (the minimum does not depend on arrival order)
//   n_violated   the count of the flag bytes, by the second kernel (integer adds)
//   a, b, c      one evaluation of the three rows at the minimal key, by the second kernel
// The common path -- a satisfied system -- issues no atomic and no flag store.
#include <algorithm>

#include "../../include/ringsnark_amd/r1cs_check.h"
#include "witness_eval.hpp"

namespace rs {

// rows whose load chains one lane keeps in flight (eval_rows_pair).  Measured on the four shapes of DESIGN.md "R1CS satisfaction
// check": 2 beats 4 by 8-17 % and 8 by 35 % -- the kernel keeps six results per row in registers (FP64: 72 VGPRs at 2, seven waves
// per SIMD; 116 at 4, 205 at 8; Montgomery: 102 at 2, four waves), and resident waves hide the row_ptr -> col -> assignment chains better than longer batches.
constexpr int CHECK_R = 2;

// device side of the report: [0] key of the first violation (all ones: none), [1] violated rows, [2..4] a, b, c there
constexpr int CHECK_WORDS = 5;

// grid: (slot chunks of 256 slot pairs) x (row groups of `rpw` rows), one dimension, ordered by xcd_position (witness_eval.hpp).
// A thread owns one slot pair (16-byte loads of the assignment) and walks the rows of its group CHECK_R at a time.
template <class M>
__global__ void __launch_bounds__(256)
r1cs_check_kernel(const uint32_t *__restrict__ rp_a, const uint32_t *__restrict__ col_a, const typename ArithOf<M>::T *__restrict__ cf_a,
                  size_t nnz_a, const int32_t *__restrict__ px_a, const uint32_t *__restrict__ rp_b,
                  const uint32_t *__restrict__ col_b, const typename ArithOf<M>::T *__restrict__ cf_b, size_t nnz_b,
                  const int32_t *__restrict__ px_b, const uint32_t *__restrict__ rp_c, const uint32_t *__restrict__ col_c,
                  const typename ArithOf<M>::T *__restrict__ cf_c, size_t nnz_c, const int32_t *__restrict__ px_c,
                  const typename ArithOf<M>::T *__restrict__ ptab, const uint64_t *__restrict__ asg, size_t m, int N, int L,
                  unsigned n_inputs, const M *__restrict__ qmod, unsigned n_groups, unsigned rpw, uint8_t *__restrict__ flags,
                  unsigned long long *__restrict__ first) {
  using T = typename ArithOf<M>::T;
  const unsigned pos = xcd_position(blockIdx.x, gridDim.x);
  const unsigned chunk = pos / n_groups, group = pos % n_groups;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)chunk * 256 + threadIdx.x;
  if (2 * pair >= S) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const size_t row_lo = (size_t)group * rpw, row_hi = row_lo + rpw < m ? row_lo + rpw : m;
  for (size_t r0 = row_lo; r0 < row_hi; r0 += CHECK_R) {
    T a0[CHECK_R], a1[CHECK_R], b0[CHECK_R], b1[CHECK_R], c0[CHECK_R], c1[CHECK_R];
    eval_rows_pair<M, CHECK_R>(rp_a, col_a, cf_a + (size_t)limb * nnz_a, r0, 1, row_hi, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, a0, a1, px_a, ptab);
    eval_rows_pair<M, CHECK_R>(rp_b, col_b, cf_b + (size_t)limb * nnz_b, r0, 1, row_hi, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, b0, b1, px_b, ptab);
    eval_rows_pair<M, CHECK_R>(rp_c, col_c, cf_c + (size_t)limb * nnz_c, r0, 1, row_hi, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, c0, c1, px_c, ptab);
#pragma unroll
    for (int j = 0; j < CHECK_R; j++) {
      // two canonical residues: one operand centred, as the dyadic product of rs_core.hip (rows past row_hi: 0 * 0 == 0)
      const bool bad0 = canon(mulmod_dd(a0[j], center(b0[j], mod), mod), mod) != c0[j];
      const bool bad1 = canon(mulmod_dd(a1[j], center(b1[j], mod), mod), mod) != c1[j];
      const unsigned long long bad = __ballot(bad0 || bad1);
      if (bad == 0ull) continue;  // wave-uniform: the common path ends here
      // the lanes of a wave hold one row and ascending slot pairs: the lowest violating lane has the wave's smallest key
      if ((int)(threadIdx.x & 63u) == __ffsll(bad) - 1) {
        const size_t row = r0 + j;
        flags[row] = 1;
        atomicMin(first, (unsigned long long)(row * S + 2 * pair + (bad0 ? 0 : 1)));
      }
    }
  }
}

// the epilogue: counts the flag bytes and evaluates the three rows once at the first violation
template <class M>
__global__ void __launch_bounds__(256)
r1cs_check_finish_kernel(const uint32_t *__restrict__ rp_a, const uint32_t *__restrict__ col_a,
                         const typename ArithOf<M>::T *__restrict__ cf_a, size_t nnz_a, const int32_t *__restrict__ px_a,
                         const uint32_t *__restrict__ rp_b, const uint32_t *__restrict__ col_b,
                         const typename ArithOf<M>::T *__restrict__ cf_b, size_t nnz_b, const int32_t *__restrict__ px_b,
                         const uint32_t *__restrict__ rp_c, const uint32_t *__restrict__ col_c,
                         const typename ArithOf<M>::T *__restrict__ cf_c, size_t nnz_c, const int32_t *__restrict__ px_c,
                         const typename ArithOf<M>::T *__restrict__ ptab, const uint64_t *__restrict__ asg, size_t m, int N, int L,
                         unsigned n_inputs, const M *__restrict__ qmod, const uint8_t *__restrict__ flags,
                         unsigned long long *__restrict__ rep /* [CHECK_WORDS] */) {
  using T = typename ArithOf<M>::T;
  __shared__ unsigned wave_count[4];
  unsigned n = 0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x) n += flags[r] ? 1u : 0u;
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if ((threadIdx.x & 63u) == 0) wave_count[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const unsigned total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
  if (total) atomicAdd(rep + 1, (unsigned long long)total);
  const unsigned long long key = rep[0];  // final: written by the launch before this one
  if (blockIdx.x != 0 || key == ~0ull) return;
  const size_t S = (size_t)L * N, row = (size_t)(key / S), idx = (size_t)(key % S), pair = idx >> 1;
  const int limb = (int)(idx / (size_t)N);
  const M mod = qmod[limb];
  T x0, x1;
  eval_row_pair<M>(rp_a, col_a, cf_a + (size_t)limb * nnz_a, row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, px_a, ptab);
  rep[2] = to_res((idx & 1) ? x1 : x0);
  eval_row_pair<M>(rp_b, col_b, cf_b + (size_t)limb * nnz_b, row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, px_b, ptab);
  rep[3] = to_res((idx & 1) ? x1 : x0);
  eval_row_pair<M>(rp_c, col_c, cf_c + (size_t)limb * nnz_c, row, asg, S, pair, RS_EVAL_FULL, n_inputs, mod, x0, x1, px_c, ptab);
  rep[4] = to_res((idx & 1) ? x1 : x0);
}

template <class M>
static void r1cs_check_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_asg, uint8_t *flags, unsigned long long *rep,
                           hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const size_t S = ctx->ring_words(), m = cs->m;
  const size_t chunks = (S / 2 + 255) / 256;
  // rows per workgroup: as many as leave the device a few waves of workgroups (a group's rows share their wires in L1;
  // 8 / 16 / 32 measured within 4 % of each other, in opposite orders on the wide and the chain circuit)
  size_t rpw = 16;
  while (rpw > (size_t)CHECK_R && chunks * ((m + rpw - 1) / rpw) < 4096) rpw >>= 1;
  const size_t groups = (m + rpw - 1) / rpw;
  RS_REQUIRE(chunks * groups < ((size_t)1 << 31), "constraint system too large for one launch of the check");
  const T *cf[3], *ptab = reinterpret_cast<const T *>(cs->d_ptab);
  for (int w = 0; w < 3; w++) cf[w] = reinterpret_cast<const T *>(cs->d_coeff[w]);
  double nnz = 0;
  for (int w = 0; w < 3; w++) nnz += (double)cs->nnz[w];
  {
    // algorithmic bytes: the assignment once (every wire is read by some row) and the three CSRs once
    ProfScope p(ctx, st, "r1cs_check", (double)cs->n_vars * S * 8 + nnz * (4 + 8.0 * ctx->L) + 3.0 * (m + 1) * 4, 7.0 * (nnz + m) * S);
    hipLaunchKernelGGL(r1cs_check_kernel<M>, dim3((unsigned)(chunks * groups)), dim3(256), 0, st, cs->d_row_ptr[0], cs->d_col[0], cf[0],
                       cs->nnz[0], cs->d_pidx[0], cs->d_row_ptr[1], cs->d_col[1], cf[1], cs->nnz[1], cs->d_pidx[1], cs->d_row_ptr[2],
                       cs->d_col[2], cf[2], cs->nnz[2], cs->d_pidx[2], ptab, d_asg, m, ctx->N, ctx->L, (unsigned)cs->n_inputs,
                       CtxArith<M>::qmod(ctx), (unsigned)groups, (unsigned)rpw, flags, rep);
  }
  RS_HIP(hipGetLastError());
  const unsigned fin_blocks = (unsigned)std::min<size_t>((m + 255) / 256, 64);
  hipLaunchKernelGGL(r1cs_check_finish_kernel<M>, dim3(fin_blocks), dim3(256), 0, st, cs->d_row_ptr[0], cs->d_col[0], cf[0], cs->nnz[0],
                     cs->d_pidx[0], cs->d_row_ptr[1], cs->d_col[1], cf[1], cs->nnz[1], cs->d_pidx[1], cs->d_row_ptr[2], cs->d_col[2],
                     cf[2], cs->nnz[2], cs->d_pidx[2], ptab, d_asg, m, ctx->N, ctx->L, (unsigned)cs->n_inputs, CtxArith<M>::qmod(ctx),
                     flags, rep);
  RS_HIP(hipGetLastError());
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_r1cs_check(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_assignment, uint8_t *d_row_flags, rs_r1cs_report *h_report,
                  rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(cs && d_assignment && h_report, "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  const size_t m = cs->m, words = ctx->ring_words();
  rs_r1cs_report out{};
  out.first_row = m;
  if (m && words) {
    hipStream_t st = S(stream);
    WsScope ws_scope(ctx, st);
    // workspace: the report words, then (unless the caller brought them) the flag bytes
    char *ws = (char *)ws_get(ctx, WS_SMALL, std::max<size_t>(256, 64 + (d_row_flags ? 0 : m)));
    unsigned long long *rep = (unsigned long long *)ws;
    uint8_t *flags = d_row_flags ? d_row_flags : (uint8_t *)(ws + 64);
    RS_HIP(hipMemsetAsync(rep, 0, sizeof(unsigned long long) * CHECK_WORDS, st));
    RS_HIP(hipMemsetAsync(rep, 0xFF, sizeof(unsigned long long), st));
    RS_HIP(hipMemsetAsync(flags, 0, m, st));
    dispatch_arith(ctx, [&](auto tag) { r1cs_check_run<decltype(tag)>(ctx, cs, d_assignment, flags, rep, st); });
    unsigned long long h[CHECK_WORDS];
    RS_HIP(hipMemcpyAsync(h, rep, sizeof(h), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    out.n_violated = h[1];
    if (h[0] != ~0ull) {
      const size_t idx = (size_t)(h[0] % words);
      out.first_row = (uint64_t)(h[0] / words);
      out.first_limb = (uint32_t)(idx / (size_t)ctx->N);
      out.first_slot = (uint32_t)(idx % (size_t)ctx->N);
      out.a = h[2];
      out.b = h[3];
      out.c = h[4];
    }
  } else if (d_row_flags && m) {
    RS_HIP(hipMemsetAsync(d_row_flags, 0, m, S(stream)));
    RS_HIP(hipStreamSynchronize(S(stream)));
  }
  *h_report = out;
  RS_API_END
}

}  // extern "C"
