// verify.hip -- groth16::verifier (zk_proof_systems/groth16/groth16.tcc:117-170) and rinocchio::verifier
// (zk_proof_systems/rinocchio/rinocchio.tcc:192-295) on the device, and the one primitive they need that the library
// did not have: the PUBLIC columns of the instance map at a point (rs_io_eval_at).
//
// Both verifiers evaluate the constraints on `primary || zeros`, interpolate and run Horner at s.  That value is
//     v_io(s) = sum_{k <= n_inputs} x_k * A_k(s),   A_k(s) = sum_j A[j][k] * u_j(s),   x_0 = 1
// (interpolation and evaluation are linear, the ring is commutative), so a verification key holds the n_inputs + 1 columns
// A_k(s), B_k(s), C_k(s) and Z(s), and a verification is a decode plus one small kernel.  There is one verifier per scheme:
// verify_members takes a batch of proofs against one key (verify_batch.h), and the single entry points (verify.h,
// modswitch.h) are a batch of one.  A key is only read; what a call writes lives in the context's workspace.
//
// rs_io_eval_at never holds the m Lagrange values of a slot at once.  With d_j = s - j and tiles of IO_TILE rows:
//   1. tile_prod_kernel   P_t = prod_{j in tile t} d_j                                            [tiles][L][N]
//   2. tile_scan_kernel   O_t = prod_{t' != t} P_t' (suffix pass, then prefix pass), Z(s) = prod_t P_t   [tiles][L][N]
//   3. io_eval_kernel     per tile: u_j = c_j * O_t * prod_{i in tile, i != j} d_i by the same suffix / prefix passes inside
//                         the tile (sub-blocks of IO_SUB rows, their values in LDS); the rows of the three CSRs are walked
//                         as the u_j appear and every term on a public column adds coeff * u_j to that column's sum.
// No division: a slot in which s equals a node gives the residues the product formula gives (evaluation_domain.tcc:28-39).
// Partial sums of different workgroups meet in the output by MODULAR addition (a compare-and-swap loop on canonical
// residues): associative and commutative, so the result does not depend on the order of arrival.
#include <algorithm>
#include <cstring>
#include <utility>

#include "../../include/ringsnark_amd/modswitch.h"
#include "../../include/ringsnark_amd/verify.h"
#include "../../include/ringsnark_amd/verify_batch.h"
#include "witness_eval.hpp"

namespace rs {

constexpr int IO_TILE = 64;    // rows per tile: the workspace is 2 * ceil(m / IO_TILE) ring elements
constexpr int IO_SUB = 8;      // rows per sub-block of a tile (IO_TILE / IO_SUB sub-blocks)
constexpr int IO_NSUB = IO_TILE / IO_SUB;
constexpr int IO_THREADS = 64; // slots per workgroup of io_eval_kernel: one wave, every lane works on its own LDS cells
constexpr int IO_KB = 8;       // public columns per workgroup (3 * IO_KB sums per slot in LDS); more columns: more batches

// the ring value of a row index j < m < q (a data value of the arithmetic)
__device__ __forceinline__ double row_val(size_t j, const Mod &) { return (double)j; }
__device__ __forceinline__ uint64_t row_val(size_t j, const ModI &) { return (uint64_t)j; }

// d_j = s - j, |d_j| <= p/2 (sv: the centred s)
template <class M>
__device__ __forceinline__ typename ArithOf<M>::T node_diff(typename ArithOf<M>::T sv, size_t j, const M &mod) {
  return reduce(subm(sv, row_val(j, mod), mod), mod);
}

// P[t][i] = prod_{j in tile t} (s_i - j).  grid (slot chunks of 256, tiles)
template <class M>
__global__ void __launch_bounds__(256)
tile_prod_kernel(const uint64_t *__restrict__ s, uint64_t *__restrict__ P, size_t m, int N, size_t S, const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const M mod = qmod[i / (size_t)N];
  const T sv = center(from_res<T>(s[i]), mod);
  const size_t j0 = (size_t)blockIdx.y * IO_TILE, j1 = j0 + IO_TILE < m ? j0 + IO_TILE : m;
  T p = T(1);
  for (size_t j = j0; j < j1; j++) p = mulmod_dd(p, node_diff<M>(sv, j, mod), mod);
  P[(size_t)blockIdx.y * S + i] = to_res(canon(p, mod));
}

// O[t][i] = prod_{t' != t} P[t'][i] (the suffix products parked in O, then a running prefix), Zt = prod_t P[t];
// hit[0] / hit[1] = min / max over the slots of the node the slot equals (0xFFFFFFFF: none), as lagrange_kernel reports it:
// s - j = 0 mod q with j < m < q  <=>  the canonical residue of s is j.
template <class M>
__global__ void __launch_bounds__(64)
tile_scan_kernel(const uint64_t *__restrict__ s, const uint64_t *__restrict__ P, uint64_t *__restrict__ O, uint64_t *__restrict__ Zt,
                 unsigned *__restrict__ hit, size_t m, size_t tiles, int N, size_t S, const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const M mod = qmod[i / (size_t)N];
  T suf = T(1);
  for (size_t t = tiles; t-- > 0;) {
    O[t * S + i] = to_res(canon(suf, mod));
    suf = mulmod_dd(suf, center(from_res<T>(P[t * S + i]), mod), mod);
  }
  if (Zt) Zt[i] = to_res(canon(suf, mod));
  T pre = T(1);
  for (size_t t = 0; t < tiles; t++) {
    O[t * S + i] = to_res(canon(mulmod_dd(pre, center(from_res<T>(O[t * S + i]), mod), mod), mod));
    pre = mulmod_dd(pre, center(from_res<T>(P[t * S + i]), mod), mod);
  }
  const uint64_t sc = s[i];
  const unsigned my_hit = sc < (uint64_t)m ? (unsigned)sc : 0xFFFFFFFFu;
  atomicMin(&hit[0], my_hit);
  atomicMax(&hit[1], my_hit);
}

// *addr = (*addr + v) mod p on canonical residues, atomically: the sum of the partial results of all workgroups, whatever
// their order
template <class M>
__device__ __forceinline__ void atomic_add_mod(uint64_t *addr, uint64_t v, const M &mod) {
  using T = typename ArithOf<M>::T;
  unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
  unsigned long long assumed = 0ull, next = v;
  for (;;) {
    const unsigned long long old = atomicCAS(a, assumed, next);
    if (old == assumed) return;
    assumed = old;
    next = to_res(canon(addm(from_res<T>((uint64_t)old), from_res<T>(v), mod), mod));
  }
}

template <class T>
struct IoCsr {
  const uint32_t *rp[3], *col[3];
  const T *cf[3];  // [L][nnz]
  const int32_t *pidx[3];
  size_t nnz[3];
  uint64_t *out[3];  // [n_inputs+1][S], zero before the launch; null: matrix not wanted
};

// grid.x = (slot chunks of IO_THREADS) x (groups of tiles), grid.y = batches of IO_KB public columns.
// LDS per lane: IO_NSUB sub-block suffixes, IO_SUB row values, 3 * kb column sums -- cell c of lane l at [c * IO_THREADS + l].
template <class M>
__global__ void __launch_bounds__(IO_THREADS)
io_eval_kernel(IoCsr<typename ArithOf<M>::T> cs, const typename ArithOf<M>::T *__restrict__ ptab, const uint64_t *__restrict__ s,
               const typename ArithOf<M>::T *__restrict__ cj /* [L][m] */, const uint64_t *__restrict__ O, size_t m, size_t tiles, int N,
               size_t S, const M *__restrict__ qmod, unsigned n_groups, unsigned tiles_per_group, unsigned n_cols, unsigned kb) {
  using T = typename ArithOf<M>::T;
  extern __shared__ unsigned long long io_lds[];
  const unsigned lane = threadIdx.x;
  T *sub_suf = reinterpret_cast<T *>(io_lds) + lane;        // [IO_NSUB]
  T *row_u = sub_suf + IO_NSUB * IO_THREADS;                // [IO_SUB]
  T *acc = row_u + IO_SUB * IO_THREADS;                     // [3][kb]
  const size_t chunk = blockIdx.x / n_groups, group = blockIdx.x % n_groups;
  const unsigned k0 = blockIdx.y * IO_KB, kn = n_cols - k0 < kb ? n_cols - k0 : kb;
  const size_t i_raw = chunk * IO_THREADS + lane;
  const bool active = i_raw < S;
  const size_t i = active ? i_raw : S - 1;  // lanes past the end work on a copy of the last slot (the wave votes as one) and store nothing
  const size_t limb = i / (size_t)N;
  const M mod = qmod[limb];
  const T sv = center(from_res<T>(s[i]), mod);
  for (unsigned a = 0; a < 3 * kb; a++) acc[a * IO_THREADS] = T(0);
  const size_t t_lo = group * tiles_per_group, t_hi = t_lo + tiles_per_group < tiles ? t_lo + tiles_per_group : tiles;
  for (size_t t = t_lo; t < t_hi; t++) {
    const size_t j0 = t * IO_TILE;
    // suffix products of the sub-blocks of this tile
    {
      T q = T(1);
      for (int b = IO_NSUB - 1; b >= 0; b--) {
        sub_suf[b * IO_THREADS] = reduce(q, mod);
#pragma unroll
        for (int r = IO_SUB - 1; r >= 0; r--) {
          const size_t j = j0 + (size_t)b * IO_SUB + r;
          if (j < m) q = mulmod_dd(q, node_diff<M>(sv, j, mod), mod);
        }
      }
    }
    T X = center(from_res<T>(O[t * S + i]), mod);  // everything outside the tile, then times the d_j passed
    for (int b = 0; b < IO_NSUB; b++) {
      const size_t jb = j0 + (size_t)b * IO_SUB;
      if (jb >= m) break;
      const size_t je = jb + IO_SUB < m ? jb + IO_SUB : m;
      uint32_t e_lo[3], e_hi[3];
#pragma unroll
      for (int w = 0; w < 3; w++) {
        e_lo[w] = cs.out[w] ? cs.rp[w][jb] : 0u;
        e_hi[w] = cs.out[w] ? cs.rp[w][je] : 0u;
      }
      {
        T y = sub_suf[b * IO_THREADS];
#pragma unroll
        for (int r = IO_SUB - 1; r >= 0; r--) {
          row_u[r * IO_THREADS] = y;
          if (jb + r < m) y = reduce(mulmod_dd(y, node_diff<M>(sv, jb + r, mod), mod), mod);
        }
      }
#pragma unroll
      for (int r = 0; r < IO_SUB; r++) {
        const size_t j = jb + r;
        if (j < m) {
          const T v = mulmod_dd(X, row_u[r * IO_THREADS], mod);
          row_u[r * IO_THREADS] = mulmod(v, cj[limb * m + j], mod);  // u_j
          X = mulmod_dd(X, node_diff<M>(sv, j, mod), mod);
        }
      }
      // the terms of rows [jb, je) on this batch's columns: the lanes look at 64 CSR entries at a time
#pragma unroll
      for (int w = 0; w < 3; w++) {
        for (uint32_t e0 = e_lo[w]; e0 < e_hi[w]; e0 += 64) {
          const uint32_t e = e0 + lane;
          const uint32_t kc = e < e_hi[w] ? cs.col[w][e] : 0xFFFFFFFFu;
          unsigned long long todo = __ballot(kc - k0 < kn);
          while (todo) {
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t ee = e0 + (uint32_t)bit;
            const uint32_t kk = (uint32_t)__shfl((int)kc, bit) - k0;
            int r = 0;
            while (cs.rp[w][jb + r + 1] <= ee) r++;  // ee < rp[je]: ends at a row of the sub-block
            T cf = cs.cf[w][limb * cs.nnz[w] + ee];
            if (cs.pidx[w]) {
              const int32_t pk = cs.pidx[w][ee];
              if (pk >= 0) cf = ptab[(size_t)pk * S + i];
            }
            T *a = acc + (size_t)(w * kb + kk) * IO_THREADS;
            *a = reduce(addm(*a, mulmod(row_u[r * IO_THREADS], cf, mod), mod), mod);
          }
        }
      }
    }
  }
  if (!active) return;
  for (int w = 0; w < 3; w++) {
    if (!cs.out[w]) continue;
    for (unsigned k = 0; k < kn; k++) {
      const uint64_t v = to_res(canon(acc[(size_t)(w * kb + k) * IO_THREADS], mod));
      if (v) atomic_add_mod<M>(cs.out[w] + (size_t)(k0 + k) * S + i_raw, v, mod);
    }
  }
}

template <class M>
static void io_eval_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *const outs[3], uint64_t *d_Zt, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const size_t m = cs->m, S = ctx->ring_words(), tiles = (m + IO_TILE - 1) / IO_TILE, n_cols = cs->n_inputs + 1;
  const int N = ctx->N;
  RS_REQUIRE(m < 0xFFFFFFFFull && tiles < 65536, "constraint system too large for the evaluation at a point");
  std::vector<uint64_t> hc;
  lagrange_constants<M>(ctx, m, hc);
  uint64_t *P = (uint64_t *)ws_get(ctx, WS_PASS_A, tiles * S * sizeof(uint64_t));
  uint64_t *O = (uint64_t *)ws_get(ctx, WS_PASS_B, tiles * S * sizeof(uint64_t));
  char *small = (char *)ws_get(ctx, WS_SMALL, 256 + hc.size() * sizeof(uint64_t));
  unsigned *d_hit = (unsigned *)small;
  T *d_c = (T *)(small + 256);
  const unsigned hit0[2] = {0xFFFFFFFFu, 0u};
  unsigned hit[2];
  RS_HIP(hipMemcpyAsync(d_hit, hit0, sizeof(hit0), hipMemcpyHostToDevice, st));
  RS_HIP(hipMemcpyAsync(d_c, hc.data(), hc.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  const M *qmod = CtxArith<M>::qmod(ctx);
  {
    ProfScope p(ctx, st, "io_tile_prod", (double)S * 8 * (1 + tiles), 7.0 * m * S);
    hipLaunchKernelGGL(tile_prod_kernel<M>, dim3((unsigned)((S + 255) / 256), (unsigned)tiles), dim3(256), 0, st, d_s, P, m, N, S, qmod);
  }
  RS_HIP(hipGetLastError());
  {
    ProfScope p(ctx, st, "io_tile_scan", (double)S * 8 * (2 + 4 * tiles), 7.0 * 3 * tiles * S);
    hipLaunchKernelGGL(tile_scan_kernel<M>, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, d_s, P, O, d_Zt, d_hit, m, tiles, N, S, qmod);
  }
  RS_HIP(hipGetLastError());
  RS_HIP(hipMemcpyAsync(hit, d_hit, sizeof(hit), hipMemcpyDeviceToHost, st));
  RS_HIP(hipStreamSynchronize(st));  // hc, hit
  // evaluation_domain.tcc:24-26: rejected only when s equals a domain element AS A RING ELEMENT
  if (hit[0] == hit[1] && hit[0] != 0xFFFFFFFFu) throw Error(RS_ERR_NOT_INVERTIBLE, "t cannot be one of the values in the domain");
  if (!outs[0] && !outs[1] && !outs[2]) return;
  IoCsr<T> a;
  double nnz = 0;
  for (int w = 0; w < 3; w++) {
    a.rp[w] = cs->d_row_ptr[w];
    a.col[w] = cs->d_col[w];
    a.cf[w] = reinterpret_cast<const T *>(cs->d_coeff[w]);
    a.pidx[w] = cs->d_pidx[w];
    a.nnz[w] = cs->nnz[w];
    a.out[w] = cs->nnz[w] ? outs[w] : nullptr;  // a matrix without entries: its columns are zero
    if (outs[w]) RS_HIP(hipMemsetAsync(outs[w], 0, n_cols * S * sizeof(uint64_t), st));
    nnz += (double)cs->nnz[w];
  }
  const unsigned kb = (unsigned)std::min<size_t>(n_cols, IO_KB), batches = (unsigned)((n_cols + IO_KB - 1) / IO_KB);
  const size_t chunks = (S + IO_THREADS - 1) / IO_THREADS;
  // tiles of one workgroup (one wave): two (the column sums are set up and added into the output once per workgroup), or
  // as many as keep the launch within about 2^15 workgroups -- many short workgroups fill the device evenly and let the CSR
  // reads of one wave hide behind the arithmetic of the others
  size_t tpg = 2;
  while (chunks * batches * ((tiles + tpg - 1) / tpg) > 32768 && tpg < tiles) tpg <<= 1;
  const size_t groups = (tiles + tpg - 1) / tpg;
  RS_REQUIRE(chunks * groups < ((size_t)1 << 31) && batches < 65536, "constraint system too large for the evaluation at a point");
  const size_t lds = (size_t)(IO_NSUB + IO_SUB + 3 * kb) * IO_THREADS * sizeof(T);
  {
    // algorithmic bytes: s and the tile products once per slot, the three CSRs once; five modular products per row and slot
    ProfScope p(ctx, st, "io_eval_at", (double)S * 8 * (1 + tiles + 3.0 * n_cols) + nnz * (4 + 8.0 * ctx->L) + 3.0 * (m + 1) * 4 + 8.0 * ctx->L * m,
                7.0 * 5 * m * S * batches);
    hipLaunchKernelGGL(io_eval_kernel<M>, dim3((unsigned)(chunks * groups), batches), dim3(IO_THREADS), lds, st, a,
                       reinterpret_cast<const T *>(cs->d_ptab), d_s, d_c, O, m, tiles, N, S, qmod, (unsigned)groups, (unsigned)tpg,
                       (unsigned)n_cols, kb);
  }
  RS_HIP(hipGetLastError());
  RS_HIP(hipStreamSynchronize(st));
}

// ---- the verification kernels ----------------------------------------------------------------------------------------
constexpr int VERIFY_WORDS = 9;  // device side of a proof's report: [0] COMPLEMENT of the key of the first failure (zero: none), [1..6] n_bad, [7] lhs, [8] rhs

struct VerifyArgs {
  const uint64_t *io[3];   // [n_inputs+1][S] public columns of A, B, C at s
  const uint64_t *Zt;      // rinocchio
  const uint64_t *el[5];   // groth16: alpha, beta, delta; rinocchio: alpha, beta, r_v, r_w, r_y
  const uint64_t *primary; // [batch][n_inputs][S]
  const uint64_t *dec;     // [batch][3 | 9][S] decoded proof elements
  unsigned n_inputs;
};

// data x data product of two canonical residues (one operand centred, as the dyadic product of rs_core.hip)
template <class M>
__device__ __forceinline__ typename ArithOf<M>::T mul_cc(typename ArithOf<M>::T a, typename ArithOf<M>::T b, const M &mod) {
  return mulmod_dd(center(a, mod), b, mod);
}

// A verification of one slot is two parts: the public sums v_io(s), w_io(s), y_io(s) = column 0 + sum_k x_k * column k
// (canonical residues), and the checks given those sums and the decoded proof elements.  verify_batch_kernel computes the
// sums of several proofs side by side and then makes the checks of each; its finish kernel does both for one slot of one
// proof (verify_slot).
template <class M>
__device__ __forceinline__ void io_sums(const VerifyArgs &a, const uint64_t *__restrict__ primary, size_t S, size_t i, const M &mod,
                                        typename ArithOf<M>::T (&io)[3]) {
  using T = typename ArithOf<M>::T;
  auto ld = [&](const uint64_t *p) { return from_res<T>(p[i]); };
#pragma unroll
  for (int w = 0; w < 3; w++) {
    T acc = ld(a.io[w]);
    for (unsigned k = 0; k < a.n_inputs; k++)
      acc = reduce(addm(acc, mul_cc<M>(ld(primary + (size_t)k * S), ld(a.io[w] + (size_t)(k + 1) * S), mod), mod), mod);
    io[w] = canon(acc, mod);
  }
}

// The checks of one slot: canonical residues lhs[c], rhs[c] of check c (verify.h).  SCHEME 0: groth16 (1 check), 1: rinocchio (6).
// dec: [3 | 9][S] decoded elements of the proof, io: its public sums at this slot.
template <class M, int SCHEME>
__device__ __forceinline__ void verify_checks(const VerifyArgs &a, const uint64_t *__restrict__ dec, size_t S, size_t i, const M &mod,
                                              const typename ArithOf<M>::T (&io)[3], uint64_t (&lhs)[6], uint64_t (&rhs)[6]) {
  using T = typename ArithOf<M>::T;
  auto ld = [&](const uint64_t *p) { return from_res<T>(p[i]); };
  if (SCHEME == 0) {
    const T A = ld(dec), B = ld(dec + S), C = ld(dec + 2 * S);
    const T alpha = ld(a.el[0]), beta = ld(a.el[1]), delta = ld(a.el[2]);
    // f = beta v_io + alpha w_io + y_io  (= gamma * (f / gamma): groth16.tcc:159-166 for an invertible gamma)
    const T f = reduce(addm(reduce(addm(mul_cc<M>(beta, io[0], mod), mul_cc<M>(alpha, io[1], mod), mod), mod), io[2], mod), mod);
    const T r = addm(reduce(addm(mul_cc<M>(alpha, beta, mod), f, mod), mod), mul_cc<M>(delta, C, mod), mod);
    lhs[0] = to_res(canon(mul_cc<M>(A, B, mod), mod));
    rhs[0] = to_res(canon(r, mod));
  } else {
    const T alpha = ld(a.el[0]), beta = ld(a.el[1]);
    T x[9];
#pragma unroll
    for (int e = 0; e < 9; e++) x[e] = ld(dec + (size_t)e * S);
#pragma unroll
    for (int c = 0; c < 4; c++) {  // V', W', Y', H' against alpha * V, W, Y, H
      lhs[c] = to_res(x[2 * c + 1]);
      rhs[c] = to_res(canon(mul_cc<M>(x[2 * c], alpha, mod), mod));
    }
    T l = reduce(addm(mul_cc<M>(x[0], ld(a.el[2]), mod), mul_cc<M>(x[2], ld(a.el[3]), mod), mod), mod);
    l = canon(addm(l, mul_cc<M>(x[4], ld(a.el[4]), mod), mod), mod);
    lhs[4] = to_res(canon(mul_cc<M>(l, beta, mod), mod));
    rhs[4] = to_res(x[8]);
    const T pv = canon(addm(x[0], io[0], mod), mod), pw = canon(addm(x[2], io[1], mod), mod), py = canon(addm(x[4], io[2], mod), mod);
    lhs[5] = to_res(canon(subm(mul_cc<M>(pv, pw, mod), py, mod), mod));
    rhs[5] = to_res(canon(mul_cc<M>(x[6], ld(a.Zt), mod), mod));
  }
}

// both parts for the proof that `a` names (a.primary, a.dec)
template <class M, int SCHEME>
__device__ __forceinline__ void verify_slot(const VerifyArgs &a, size_t S, size_t i, const M &mod, uint64_t (&lhs)[6], uint64_t (&rhs)[6]) {
  typename ArithOf<M>::T io[3];
  io_sums<M>(a, a.primary, S, i, mod, io);
  verify_checks<M, SCHEME>(a, a.dec, S, i, mod, io, lhs, rhs);
}

// Proofs whose public sums a thread carries at once.  A column of the key is read once per VERIFY_PB proofs: per proof
// (3 (n_inputs + 1) / VERIFY_PB + n_inputs) S words instead of (4 n_inputs + 3) S.  The accumulators are VERIFY_PB x 3 sums x
// 2 slots 64-bit words (48 VGPRs at 4); the checks that follow, with the other proofs' sums still live, set the kernel's
// count: 92..136 VGPRs and 3 to 5 waves per SIMD at 4, 162..184 and 2 to 3 at 8, no scratch either way.  4, not 8, by
// measurement (profiles/verify_batch.txt): a wave does the modular products of VERIFY_PB proofs one after the other, and at
// the logistic-regression shape (1024 slot pairs, 517 inputs, integer arithmetic) a batch of 64 is 16 waves x 64 / VERIFY_PB
// groups -- the kernel is bound by the products of one wave, not by the columns, and took 5.5 ms at 8 against 2.8 ms at 4;
// at the headline shape both take the same time.
constexpr int VERIFY_PB = 4;

// f(integral_constant<int, P>) for every P of the sequence: indices into a register array that are constants by construction
template <int... P, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, P...>, F &&f) {
  (f(std::integral_constant<int, P>{}), ...);
}

// the two words of a slot pair, one 16-byte load where the array is 16-byte aligned (S and the pair's first index are even)
__device__ __forceinline__ void ld_pair(const uint64_t *__restrict__ p, bool vec, uint64_t (&v)[2]) {
  if (vec) {
    const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(p);
    v[0] = t.x, v[1] = t.y;
  } else {
    v[0] = p[0], v[1] = p[1];
  }
}

// a.primary [batch][n_inputs][S], a.dec [batch][3 | 9][S]; rep [batch][VERIFY_WORDS], zero before the launch, word 0 of a
// proof: the COMPLEMENT of the key (check * S + position) of its first failure (zero: none; one memset prepares every
// word).  grid (chunks of 256 slot pairs, groups of VERIFY_PB proofs).  A thread owns a slot pair and the lanes of a wave
// hold ascending pairs: the lowest failing lane has the wave's smallest position.  skip4 bit b: check 4 is not made for
// proof b.  The tail group's guard p < nb is wave-uniform.
template <class M, int SCHEME>
__global__ void __launch_bounds__(256)
verify_batch_kernel(VerifyArgs a, int batch, unsigned long long skip4, int prim_vec, int N, size_t S, const M *__restrict__ qmod,
                    unsigned long long *__restrict__ rep) {
  using T = typename ArithOf<M>::T;
  constexpr int NE = SCHEME == 0 ? 3 : 9, NC = SCHEME == 0 ? 1 : 6;
  const size_t pair = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = 2 * pair < S;
  const size_t i = live ? 2 * pair : 0;
  const int b0 = (int)blockIdx.y * VERIFY_PB;
  const int nb = batch - b0 < VERIFY_PB ? batch - b0 : VERIFY_PB;
  const M mod = qmod[i / (size_t)N];
  T acc[VERIFY_PB][3][2];
  if (live) {
    uint64_t c[2];
#pragma unroll
    for (int w = 0; w < 3; w++) {
      ld_pair(a.io[w] + i, true, c);
#pragma unroll
      for (int p = 0; p < VERIFY_PB; p++) acc[p][w][0] = from_res<T>(c[0]), acc[p][w][1] = from_res<T>(c[1]);
    }
    const size_t pstride = (size_t)a.n_inputs * S;
    for (unsigned k = 0; k < a.n_inputs; k++) {
      T col[3][2];  // column k + 1 of the three matrices: loaded once, used by every proof of the group
#pragma unroll
      for (int w = 0; w < 3; w++) {
        ld_pair(a.io[w] + (size_t)(k + 1) * S + i, true, c);
        col[w][0] = from_res<T>(c[0]), col[w][1] = from_res<T>(c[1]);
      }
      const uint64_t *xk = a.primary + (size_t)b0 * pstride + (size_t)k * S + i;
#pragma unroll
      for (int p = 0; p < VERIFY_PB; p++) {
        if (p < nb) {
          ld_pair(xk + (size_t)p * pstride, prim_vec != 0, c);
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const T x = center(from_res<T>(c[h]), mod);
#pragma unroll
            for (int w = 0; w < 3; w++) acc[p][w][h] = reduce(addm(acc[p][w][h], mulmod_dd(x, col[w][h], mod), mod), mod);
          }
        }
      }
    }
  }
  static_for(std::make_integer_sequence<int, VERIFY_PB>{}, [&](auto pc) {
    constexpr int p = decltype(pc)::value;
    if (p < nb) {
      unsigned bad[2] = {0u, 0u};
      if (live) {
        const uint64_t *dec = a.dec + (size_t)(b0 + p) * NE * S;
        const unsigned skip = (SCHEME == 1 && ((skip4 >> (b0 + p)) & 1ull)) ? 1u << 4 : 0u;
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const T io[3] = {canon(acc[p][0][h], mod), canon(acc[p][1][h], mod), canon(acc[p][2][h], mod)};
          uint64_t lhs[6], rhs[6];
          verify_checks<M, SCHEME>(a, dec, S, i + h, mod, io, lhs, rhs);
#pragma unroll
          for (int c = 0; c < NC; c++)
            if (lhs[c] != rhs[c] && !((skip >> c) & 1u)) bad[h] |= 1u << c;
        }
      }
      unsigned long long *rp = rep + (size_t)(b0 + p) * VERIFY_WORDS;
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const bool f0 = (bad[0] >> c) & 1u, f1 = (bad[1] >> c) & 1u;
        const unsigned long long v0 = __ballot(f0), v1 = __ballot(f1);
        if ((v0 | v1) == 0ull) continue;  // wave-uniform: an accepted proof issues no atomic
        if ((int)(threadIdx.x & 63u) == __ffsll((long long)(v0 | v1)) - 1) {
          atomicAdd(rp + 1 + c, (unsigned long long)(__popcll(v0) + __popcll(v1)));
          atomicMax(rp, ~(unsigned long long)((size_t)c * S + 2 * pair + (f0 ? 0 : 1)));  // the smallest key has the largest complement
        }
      }
    }
  });
}

// the two residues at the first failure of every proof: one wave per proof
template <class M, int SCHEME>
__global__ void __launch_bounds__(64)
verify_batch_finish_kernel(VerifyArgs a, int N, size_t S, const M *__restrict__ qmod, unsigned long long *__restrict__ rep) {
  constexpr int NE = SCHEME == 0 ? 3 : 9;
  unsigned long long *rp = rep + (size_t)blockIdx.x * VERIFY_WORDS;
  const unsigned long long inv = rp[0];  // final: written by the launch before this one
  if (threadIdx.x != 0 || inv == 0ull) return;
  const unsigned long long key = ~inv;
  const size_t c = (size_t)(key / S), i = (size_t)(key % S);
  if (a.n_inputs) a.primary += (size_t)blockIdx.x * a.n_inputs * S;
  a.dec += (size_t)blockIdx.x * NE * S;
  uint64_t lhs[6] = {0, 0, 0, 0, 0, 0}, rhs[6] = {0, 0, 0, 0, 0, 0};
  verify_slot<M, SCHEME>(a, S, i, qmod[i / (size_t)N], lhs, rhs);
  rp[7] = lhs[c];
  rp[8] = rhs[c];
}

template <class M, int SCHEME>
static void verify_launch(rs_ctx *ctx, const VerifyArgs &a, int batch, unsigned long long skip4, unsigned long long *rep, hipStream_t st) {
  constexpr int NE = SCHEME == 0 ? 3 : 9, NEL = SCHEME == 0 ? 3 : 6;
  const size_t S = ctx->ring_words();
  const int groups = (batch + VERIFY_PB - 1) / VERIFY_PB;
  const int prim_vec = (reinterpret_cast<uintptr_t>(a.primary) & 15u) == 0 ? 1 : 0;
  {
    // algorithmic bytes: the columns and the key's elements once per group, its own inputs and decodings once per proof
    ProfScope p(ctx, st, SCHEME == 0 ? "groth16_verify" : "rinocchio_verify",
                (groups * (3.0 * (a.n_inputs + 1) + NEL) + (double)batch * (a.n_inputs + NE)) * S * 8,
                7.0 * (3.0 * a.n_inputs + (SCHEME == 0 ? 5 : 10)) * S * batch);
    hipLaunchKernelGGL((verify_batch_kernel<M, SCHEME>), dim3((unsigned)((S / 2 + 255) / 256), (unsigned)groups), dim3(256), 0, st, a, batch,
                       skip4, prim_vec, ctx->N, S, CtxArith<M>::qmod(ctx), rep);
  }
  RS_HIP(hipGetLastError());
  hipLaunchKernelGGL((verify_batch_finish_kernel<M, SCHEME>), dim3((unsigned)batch), dim3(64), 0, st, a, ctx->N, S, CtxArith<M>::qmod(ctx), rep);
  RS_HIP(hipGetLastError());
}

// A verification key of either scheme: device copies of everything a verification reads.  No verification writes to it.
struct VkBase {
  rs_ctx *ctx = nullptr;      // compared at every use, never dereferenced through the key
  int device = 0;
  int scheme = 0;             // 0 groth16, 1 rinocchio
  size_t n_inputs = 0, words = 0;
  uint64_t *d_mem = nullptr;  // one allocation: io [3][n_inputs+1][S], Zt [S], el [5][S], sk [K][N_enc]
  uint64_t *io[3] = {nullptr, nullptr, nullptr}, *Zt = nullptr, *el[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  uint64_t *sk = nullptr;
};

}  // namespace rs

using namespace rs;

// rs_groth16_vk / rs_rinocchio_vk are opaque names of a VkBase (the scheme is checked at every use)
template <class VK>
static const VkBase *vk_of(const VK *vk) { return reinterpret_cast<const VkBase *>(vk); }

static void io_eval_at(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *d_Aio, uint64_t *d_Bio, uint64_t *d_Cio,
                       uint64_t *d_Zt, hipStream_t st) {
  RS_REQUIRE(cs && d_s, "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  RS_REQUIRE(cs->m >= 1, "empty constraint system");
  uint64_t *const outs[3] = {d_Aio, d_Bio, d_Cio};
  WsScope ws_scope(ctx, st);
  dispatch_arith(ctx, [&](auto tag) { io_eval_run<decltype(tag)>(ctx, cs, d_s, outs, d_Zt, st); });
}

static void vk_free(VkBase *vk) {
  if (!vk) return;
  if (vk->d_mem) {
    // Called from the destroy entry points, which report nothing: no throwing helper here, and nothing of the context is
    // read -- a host that drops its objects in any order (a garbage collector) may have destroyed the context already.
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != vk->device) (void)hipSetDevice(vk->device);
    (void)hipMemset(vk->d_mem, 0, vk->words * sizeof(uint64_t));  // the secret material does not outlive the key
    (void)hipDeviceSynchronize();
    (void)hipFree(vk->d_mem);
    if (prev >= 0 && prev != vk->device) (void)hipSetDevice(prev);
  }
  delete vk;
}

// el: the scheme's trapdoor elements in the order of VerifyArgs::el; must_invert: an element that has to be a unit (or null)
template <class VK>
static void vk_create(rs_ctx *ctx, int scheme, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *const *el, int n_el,
                      const uint64_t *must_invert, const uint64_t *d_sk, VK **out) {
  RS_REQUIRE(cs && d_s && d_sk && out, "null argument");
  for (int e = 0; e < n_el; e++) RS_REQUIRE(el[e] != nullptr, "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  const size_t S = ctx->ring_words(), n_cols = cs->n_inputs + 1, sk_words = (size_t)ctx->K * ctx->N_enc;
  VkBase *vk = new VkBase();
  struct Guard {
    VkBase *p;
    ~Guard() { vk_free(p); }
  } guard{vk};
  vk->ctx = ctx;
  vk->device = ctx->device;
  vk->scheme = scheme;
  vk->n_inputs = cs->n_inputs;
  vk->words = (3 * n_cols + 1 + 5) * S + sk_words;
  RS_HIP(hipMalloc(&vk->d_mem, vk->words * sizeof(uint64_t)));
  uint64_t *p = vk->d_mem;
  for (int w = 0; w < 3; w++, p += n_cols * S) vk->io[w] = p;
  vk->Zt = p, p += S;
  for (int e = 0; e < 5; e++, p += S) vk->el[e] = p;
  vk->sk = p;
  RS_HIP(hipMemset(vk->d_mem, 0, vk->words * sizeof(uint64_t)));
  for (int e = 0; e < n_el; e++) RS_HIP(hipMemcpy(vk->el[e], el[e], S * sizeof(uint64_t), hipMemcpyDeviceToDevice));
  RS_HIP(hipMemcpy(vk->sk, d_sk, sk_words * sizeof(uint64_t), hipMemcpyDeviceToDevice));
  if (must_invert) {  // groth16.tcc:162 divides by gamma.  The inverse lands in the first column block, which io_eval_at clears and fills next
    const int status = rs_ring_inv(ctx, vk->io[0], must_invert, 1, nullptr);
    if (status != RS_OK) throw Error(status, rs_last_error());  // RS_ERR_NOT_INVERTIBLE, "element is not invertible in ring"
  }
  io_eval_at(ctx, cs, d_s, vk->io[0], vk->io[1], vk->io[2], vk->Zt, nullptr);
  guard.p = nullptr;
  *out = reinterpret_cast<VK *>(vk);
}

// the report from the downloaded words h [VERIFY_WORDS] of one proof
static rs_verify_report report_of(const rs_ctx *ctx, const unsigned long long *h, int NC) {
  const size_t S = ctx->ring_words();
  rs_verify_report out{};
  for (int c = 0; c < NC; c++) {
    out.n_bad[c] = h[1 + c];
    if (h[1 + c]) out.failed |= 1u << c;
  }
  out.accepted = out.failed == 0 ? 1u : 0u;
  if (h[0] != 0ull) {
    const unsigned long long key = ~h[0];  // (check * S + position) of the first failure
    const size_t idx = (size_t)(key % S);
    out.first_check = (uint32_t)(key / S);
    out.first_limb = (uint32_t)(idx / (size_t)ctx->N);
    out.first_slot = (uint32_t)(idx % (size_t)ctx->N);
    out.lhs = h[7];
    out.rhs = h[8];
  }
  return out;
}

// The verifier of either scheme (verify.h, modswitch.h, verify_batch.h): `batch` proofs of level K_lvl, d_proofs
// [batch][NE][L][2][K_lvl][N_enc] (ctx->K: unswitched proofs), against one key; the outputs as verify_batch.h has them.  The
// decodings and the report words of the whole batch live in the context's workspace, under the context's lock from the first
// decode to the download.  Returns the noise budgets [batch * NE][L] the verdicts were taken from.
template <int SCHEME>
static std::vector<int> verify_members(rs_ctx *ctx, const VkBase *vk, int K_lvl, int batch, const uint64_t *d_primary, const uint64_t *d_proofs,
                                       const int *h_empty, int *h_status, int *h_budget_min, rs_verify_report *h_reports, hipStream_t st) {
  constexpr int NE = SCHEME == 0 ? 3 : 9, NC = SCHEME == 0 ? 1 : 6;
  RS_REQUIRE(K_lvl >= 1 && K_lvl <= ctx->K, "level out of range: 1 <= K_lvl <= K");
  RS_REQUIRE(vk != nullptr, "null argument");
  RS_REQUIRE(vk->ctx == ctx, "verification key of another context");
  RS_REQUIRE(vk->scheme == SCHEME, "verification key of the other scheme");
  RS_REQUIRE(batch >= 0 && batch <= RS_VERIFY_BATCH_MAX, "batch out of range: 0 <= batch <= RS_VERIFY_BATCH_MAX");
  if (batch == 0) return {};
  RS_REQUIRE(d_proofs && h_status && h_reports, "null argument");
  RS_REQUIRE(d_primary || vk->n_inputs == 0, "null argument");
  const size_t S = ctx->ring_words(), EW = (size_t)ctx->L * 2 * K_lvl * ctx->N_enc, L = (size_t)ctx->L;
  const size_t n_el = (size_t)batch * NE;
  auto empty = [&](size_t e) { return h_empty && h_empty[e]; };
  std::vector<int> budget(n_el * L, level_bit_count(ctx, K_lvl) - 1);  // an EMPTY element keeps the budget of a noiseless ciphertext
  std::vector<unsigned long long> h((size_t)batch * VERIFY_WORDS);
  unsigned long long skip4 = 0;
  bool any_empty = false;
  for (size_t e = 0; e < n_el; e++) any_empty = any_empty || empty(e);
  if (SCHEME == 1)
    for (int b = 0; b < batch; b++)
      if (empty((size_t)b * NE + 8)) skip4 |= 1ull << b;  // rinocchio.tcc:199-206, 283-288
  {
    WsScope ws_scope(ctx, st);
    uint64_t *dec = (uint64_t *)ws_get(ctx, WS_VERIFY, (n_el * S + h.size()) * sizeof(uint64_t));
    unsigned long long *rep = reinterpret_cast<unsigned long long *>(dec + n_el * S);
    if (any_empty) RS_HIP(hipMemsetAsync(dec, 0, n_el * S * sizeof(uint64_t), st));
    // the runs of non-EMPTY elements of the flattened batch: without EMPTY elements one decode of all of them
    for (size_t e = 0; e < n_el;) {
      if (empty(e)) {
        e++;
        continue;
      }
      size_t n = 1;
      while (e + n < n_el && !empty(e + n)) n++;
      decode_held(ctx, K_lvl, vk->sk, d_proofs + e * EW, n, dec + e * S, budget.data() + e * L, st);
      e += n;
    }
    VerifyArgs a{};
    for (int w = 0; w < 3; w++) a.io[w] = vk->io[w];
    a.Zt = vk->Zt;
    for (int e = 0; e < 5; e++) a.el[e] = vk->el[e];
    a.primary = d_primary;
    a.dec = dec;
    a.n_inputs = (unsigned)vk->n_inputs;
    RS_HIP(hipMemsetAsync(rep, 0, h.size() * sizeof(unsigned long long), st));
    dispatch_arith(ctx, [&](auto tag) { verify_launch<decltype(tag), SCHEME>(ctx, a, batch, skip4, rep, st); });
    RS_HIP(hipMemcpyAsync(h.data(), rep, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
  }
  for (int b = 0; b < batch; b++) {
    const int *bb = budget.data() + (size_t)b * NE * L;
    const int lowest = *std::min_element(bb, bb + NE * L);
    // a proof with a spent budget went through the kernels like the others; its report is not given out
    h_status[b] = lowest <= 0 ? RS_ERR_NOISE : RS_OK;
    h_reports[b] = lowest <= 0 ? rs_verify_report{} : report_of(ctx, h.data() + (size_t)b * VERIFY_WORDS, NC);
    if (h_budget_min) h_budget_min[b] = lowest;
  }
  return budget;
}

// verify.h, modswitch.h: one proof is a batch of one.  A spent budget ends the call as it ends the reference's verifier, with
// the text the noise guard of rs_enc_decode has for the run of non-EMPTY elements the ciphertext was decoded in, and
// *h_report is not written.
template <int SCHEME>
static void verify(rs_ctx *ctx, int K_lvl, const VkBase *vk, const uint64_t *d_primary, const uint64_t *d_proof, const int *h_empty,
                   rs_verify_report *h_report, hipStream_t st) {
  constexpr size_t NE = SCHEME == 0 ? 3 : 9;
  RS_REQUIRE(h_report != nullptr, "null argument");
  int status = RS_OK;
  rs_verify_report report{};
  const std::vector<int> budget = verify_members<SCHEME>(ctx, vk, K_lvl, 1, d_primary, d_proof, h_empty, &status, nullptr, &report, st);
  if (status == RS_ERR_NOISE) {
    auto empty = [&](size_t e) { return h_empty && h_empty[e]; };
    const size_t L = (size_t)ctx->L;
    const size_t spent = (size_t)(std::find_if(budget.begin(), budget.end(), [](int b) { return b <= 0; }) - budget.begin());
    const size_t e = spent / L;  // the element of the first spent (element, limb)
    size_t e0 = e, e1 = e + 1;   // its run of non-EMPTY elements, [e0, e1)
    while (e0 > 0 && !empty(e0 - 1)) e0--;
    while (e1 < NE && !empty(e1)) e1++;
    throw Error(RS_ERR_NOISE, noise_message((int)(spent % L), e - e0, e1 - e0));
  }
  *h_report = report;
}

extern "C" {

int rs_io_eval_at(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *d_Aio, uint64_t *d_Bio, uint64_t *d_Cio,
                  uint64_t *d_Zt, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  io_eval_at(ctx, cs, d_s, d_Aio, d_Bio, d_Cio, d_Zt, S(stream));
  RS_API_END
}

int rs_groth16_vk_create(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                         const uint64_t *d_gamma, const uint64_t *d_delta, const uint64_t *d_sk, rs_groth16_vk **out) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(d_gamma != nullptr, "null argument");
  const uint64_t *el[3] = {d_alpha, d_beta, d_delta};
  vk_create<rs_groth16_vk>(ctx, 0, cs, d_s, el, 3, d_gamma, d_sk, out);
  RS_API_END
}
void rs_groth16_vk_destroy(rs_groth16_vk *vk) { vk_free(const_cast<VkBase *>(vk_of(vk))); }

int rs_rinocchio_vk_create(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                           const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                           rs_rinocchio_vk **out) {
  RS_API_BEGIN_CTX(ctx)
  const uint64_t *el[5] = {d_alpha, d_beta, d_rv, d_rw, d_ry};
  vk_create<rs_rinocchio_vk>(ctx, 1, cs, d_s, el, 5, nullptr, d_sk, out);
  RS_API_END
}
void rs_rinocchio_vk_destroy(rs_rinocchio_vk *vk) { vk_free(const_cast<VkBase *>(vk_of(vk))); }

int rs_groth16_verify(rs_ctx *ctx, const rs_groth16_vk *vk, const uint64_t *d_primary, const uint64_t *d_proof, const int *h_empty,
                      rs_verify_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify<0>(ctx, ctx->K, vk_of(vk), d_primary, d_proof, h_empty, h_report, S(stream));
  RS_API_END
}

int rs_rinocchio_verify(rs_ctx *ctx, const rs_rinocchio_vk *vk, const uint64_t *d_primary, const uint64_t *d_proof,
                        const int *h_empty, rs_verify_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify<1>(ctx, ctx->K, vk_of(vk), d_primary, d_proof, h_empty, h_report, S(stream));
  RS_API_END
}

// modswitch.h: the same verifiers on a proof of K_lvl primes -- only the decode differs
int rs_groth16_verify_level(rs_ctx *ctx, const rs_groth16_vk *vk, int K_lvl, const uint64_t *d_primary, const uint64_t *d_proof,
                            const int *h_empty, rs_verify_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify<0>(ctx, K_lvl, vk_of(vk), d_primary, d_proof, h_empty, h_report, S(stream));
  RS_API_END
}

int rs_rinocchio_verify_level(rs_ctx *ctx, const rs_rinocchio_vk *vk, int K_lvl, const uint64_t *d_primary, const uint64_t *d_proof,
                              const int *h_empty, rs_verify_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify<1>(ctx, K_lvl, vk_of(vk), d_primary, d_proof, h_empty, h_report, S(stream));
  RS_API_END
}

// verify_batch.h
int rs_verify_batch_group(void) { return VERIFY_PB; }

int rs_groth16_verify_batch(rs_ctx *ctx, const rs_groth16_vk *vk, int K_lvl, int batch, const uint64_t *d_primary, const uint64_t *d_proofs,
                            const int *h_empty, int *h_status, int *h_budget_min, rs_verify_report *h_reports, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify_members<0>(ctx, vk_of(vk), K_lvl, batch, d_primary, d_proofs, h_empty, h_status, h_budget_min, h_reports, S(stream));
  RS_API_END
}

int rs_rinocchio_verify_batch(rs_ctx *ctx, const rs_rinocchio_vk *vk, int K_lvl, int batch, const uint64_t *d_primary,
                              const uint64_t *d_proofs, const int *h_empty, int *h_status, int *h_budget_min, rs_verify_report *h_reports,
                              rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  verify_members<1>(ctx, vk_of(vk), K_lvl, batch, d_primary, d_proofs, h_empty, h_status, h_budget_min, h_reports, S(stream));
  RS_API_END
}

}  // extern "C"
