// witness.hip -- r1cs_to_qrp_witness_map, quasi-linear: dispatch between the launch paths, R1CS side, C ABI.
//
// The reference interpolates on the domain {0..m-1} with an O(m^2) Lagrange routine
// (util/polynomials.tcc:10-43), multiplies A*B by schoolbook and long-divides by Z
// (util/polynomials.tcc:62-81, util/evaluation_domain.tcc:54-84): ~18 m^2 ring operations.
// Every ring operation is slot-wise, so one ring limb is N independent problems over the prime
// field F_{q_i} ("columns"), and every result is a canonical residue, so ANY exact algorithm is
// bit-identical.  Per column, with M = next_pow2(m):
//
//   interpolation (values y_j at j = 0..m-1  ->  monomial coefficients):
//     1. Newton (falling-factorial) coefficients by one convolution:
//            f = (y_j / j!) * ((-1)^k / k!)                    [cyclic, length 2M]
//     2. Newton -> monomial by a product tree: node [a, a+n) holds
//            F_node = F_left + D_left * F_right,  D_left = prod_{j in left half}(x - j)
//        levels n <= 16 by schoolbook in registers, larger levels by batched length-n cyclic transforms
//        against precomputed spectra of D_left.
//   H = quo(A*B, Z) (= quo(A*B - C, Z): deg C < deg Z) through rev(H) = rev(A*B) * rev(Z)^-1 mod x^(m-1), the power
//        series rev(Z)^-1 precomputed per (prime, m).  ZK patch terms (r1cs_to_qrp.tcc:230-235) added coefficient-wise.
//
// The units of the witness map (DESIGN.md section 3 describes each kernel).  A unit instantiates the kernels of its own
// headers only and calls the other units through the host functions of witness_launch.hpp:
//   witness_plan.hip  the per-(context, m) plan (witness_plan.hpp): host-side table construction, the plan cache,
//                     the column plans (witness_cols.hpp: per-limb table pointers, ColMap).  No kernel.
//   witness_lds.hip   every kernel built on the generic LDS round functions of ntt_core.hpp (one unit: see its header)
//                       witness_tiles.hpp      M <= 2^14, one column = one LDS tile: tree_columns_kernel, interp_columns_kernel,
//                                              h_tile_kernel, h_columns_kernel
//                       witness_tree_wide.hpp  tree_wide_kernel<13 | 14>: the product tree's tiles of the multi-pass path
//                       witness_bc.hpp         ring primes without a 2M-th root of unity: pairwise and two-dimensional
//                                              block convolutions
//   witness_big.hip   M > 2^14: the multi-pass path
//                       witness_multipass.hpp  cross passes over global memory + rooted 2^13 sub-transforms (sub_ntt_wide_kernel)
//                       witness_inc.hpp        the incomplete transforms of primes without a 2M-th root of unity
//   this file         the dispatch between the three paths (launch_interp, launch_h), the chunking of columns, the R1CS
//                     handle, and the extern "C" entry points
//                       witness_eval.hpp       a14 (linear_combination::evaluate) into columns, io vectors, io / mid output
//                       witness_cols.hpp       layout transposes
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "witness_eval.hpp"
#include "witness_launch.hpp"

namespace rs {

// Interpolate `ncols` columns in place.  Column c belongs to chunk-local limb (c % S) / slots_per_limb
// (several vectors of S columns are batched); cp is shifted so that entry 0 is limb0.
template <class M>
static void launch_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *cols, size_t ncols, size_t S,
                          size_t slots_per_limb, int limb0, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  if (P->bcLog) {  // a ring prime without a 2M-th root of unity: block convolutions
    const size_t chunk = std::min(ncols, bc_chunk_cols(P));
    if constexpr (FP) {
      if (P->bc2 && chunk < ncols && g_tune.witness_tree_once) {  // the product tree's tiles in one launch (see the full-length path below)
        for (size_t c0 = 0; c0 < ncols; c0 += chunk)
          bc2_interp(ctx, P, cp, cols + c0 * P->M, std::min(chunk, ncols - c0), c0, S, slots_per_limb, limb0, st, 1);
        bc2_interp(ctx, P, cp, cols, ncols, 0, S, slots_per_limb, limb0, st, 2);
        for (size_t c0 = 0; c0 < ncols; c0 += chunk)
          bc2_interp(ctx, P, cp, cols + c0 * P->M, std::min(chunk, ncols - c0), c0, S, slots_per_limb, limb0, st, 4);
        return;
      }
    }
    for (size_t c0 = 0; c0 < ncols; c0 += chunk) {
      if constexpr (FP) {
        if (P->bc2) {
          bc2_interp(ctx, P, cp, cols + c0 * P->M, std::min(chunk, ncols - c0), c0, S, slots_per_limb, limb0, st);
          continue;
        }
      }
      bc_interp<M>(ctx, P, cp, cols + c0 * P->M, std::min(chunk, ncols - c0), c0, S, slots_per_limb, st);
    }
    return;
  }
  if constexpr (FP) {
    if (single_tile_ok(P->logM) && !P->incomplete) {
      // one launch, tile = M, two workgroups per CU: Newton conversion by the two rooted M-point
      // sub-transforms, then the product tree in place
      launch_tree_tiles(ctx, cols, ncols, 0, P->logM, P->logM, S, slots_per_limb, cp, st, true);
      return;
    }
  }
  if (P->logM <= g_tune.witness_lds_logM) {
    launch_interp_columns<M>(ctx, P, cp, cols, ncols, S, slots_per_limb, st);
    return;
  }
  const size_t chunk = std::min(ncols, big_chunk_cols(P));
  // the tile kernel also writes level 15's workspace for the right children ([ncols][M], for ALL the columns it covers)
  // when that fits beside everything else (24 GiB; a configs[3] rank is tight)
  const bool tfwd = tree_fwd_stages<M>(P) && ncols * P->M * sizeof(double) <= ((size_t)24 << 30);
  T *W = (T *)ws_get(ctx, WS_PASS_A, std::max(chunk * 2 * P->M, (tfwd && chunk < ncols && g_tune.witness_tree_once) ? ncols * P->M : 0) * sizeof(double));
  if (chunk < ncols && g_tune.witness_tree_once) {
    // the tiles of the product tree work in place on the columns: ONE launch over all of them between the sub-chunked
    // phases (tile kernels like long launches: 183.5 -> 176 ms per headline proof when every launch covers a whole chunk,
    // profiles/r05_knob_ab_big_ws.txt; the workspace-bound phases keep their 6 GiB sub-chunks, which they prefer)
    for (size_t c0 = 0; c0 < ncols; c0 += chunk)
      big_interp<M>(ctx, P, cp, cols + c0 * P->M, W, std::min(chunk, ncols - c0), c0, S, slots_per_limb, limb0, st, 1);
    big_interp<M>(ctx, P, cp, cols, W, ncols, 0, S, slots_per_limb, limb0, st, 2, tfwd);
    for (size_t c0 = 0; c0 < ncols; c0 += chunk)  // a sub-chunk's levels above the tiles work on its slice of the [ncols][M] workspace
      big_interp<M>(ctx, P, cp, cols + c0 * P->M, W + (tfwd ? c0 * P->M : 0), std::min(chunk, ncols - c0), c0, S, slots_per_limb, limb0, st, 4, tfwd);
    return;
  }
  for (size_t c0 = 0; c0 < ncols; c0 += chunk) {
    const size_t nc = std::min(chunk, ncols - c0);
    big_interp<M>(ctx, P, cp, cols + c0 * P->M, W, nc, c0, S, slots_per_limb, limb0, st, 7, tfwd);
  }
}

// H for the S columns of a chunk (A, B, H: [S][M]); `spl` columns per limb, cm locates d1..d3
template <class M>
static void launch_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A,
                     const typename ArithOf<M>::T *B, typename ArithOf<M>::T *H, size_t S, size_t spl, const uint64_t *d1,
                     const uint64_t *d2, const uint64_t *d3, const ColMap &cm, hipStream_t st,
                     const typename ArithOf<M>::T *Cc = nullptr /* coefficients of C when the call interpolates them: the coset form */) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  const size_t Mlen = P->M;
  if (P->bcLog) {
    const size_t chunk = std::min(S, bc_chunk_cols(P));
    for (size_t c0 = 0; c0 < S; c0 += chunk) {
      if constexpr (FP) {
        if (P->bc2) {
          bc2_h(ctx, P, cp, A + c0 * Mlen, B + c0 * Mlen, H + c0 * Mlen, std::min(chunk, S - c0), c0, S, spl, d1, d2, d3, cm, cm.limb0, st);
          continue;
        }
      }
      bc_h<M>(ctx, P, cp, A + c0 * Mlen, B + c0 * Mlen, H + c0 * Mlen, std::min(chunk, S - c0), c0, S, spl, d1, d2, d3, cm, st);
    }
    return;
  }
  if constexpr (FP) {
    if (single_tile_ok(P->logM) && !P->incomplete) {
      launch_h_tile(ctx, P, cp, A, B, H, S, spl, d1, d2, d3, cm, st);
      return;
    }
  }
  if (P->logM <= g_tune.witness_lds_logM) {
    launch_h_columns<M>(ctx, P, cp, A, B, H, S, spl, d1, d2, d3, cm, st);
    return;
  }
  const size_t chunk = std::min(S, big_chunk_cols(P));
  T *W1 = (T *)ws_get(ctx, WS_PASS_A, chunk * 2 * Mlen * sizeof(double));
  T *W2 = (T *)ws_get(ctx, WS_PASS_B, chunk * 2 * Mlen * sizeof(double));
  for (size_t c0 = 0; c0 < S; c0 += chunk) {
    const size_t nc = std::min(chunk, S - c0);
    if (Cc && g_tune.witness_h_coset && P->limb[cm.limb0].d_cos_z)
      big_h_coset<M>(ctx, P, cp, A + c0 * Mlen, B + c0 * Mlen, Cc + c0 * Mlen, H + c0 * Mlen, W1, W2, nc, c0, S, spl, d1, d2, d3, cm, cm.limb0, st);
    else
      big_h<M>(ctx, P, cp, A + c0 * Mlen, B + c0 * Mlen, H + c0 * Mlen, W1, W2, nc, c0, S, spl, d1, d2, d3, cm, cm.limb0, st);
  }
}

void r1cs_evaluate_run(rs_ctx *ctx, const rs_r1cs *cs, int which, int mode, const uint64_t *d_asg, uint64_t *d_out,
                       hipStream_t st) {
  const size_t S = ctx->ring_words();
  const unsigned by = (unsigned)((S / 2 + 255) / 256);
  dispatch_arith(ctx, [&](auto tag) {  // rs_r1cs holds the table constants of either arithmetic behind double pointers
    using M = decltype(tag);
    using T = typename ArithOf<M>::T;
    hipLaunchKernelGGL(r1cs_eval_kernel<M>, dim3((unsigned)cs->m, by), dim3(256), 0, st, cs->d_row_ptr[which], cs->d_col[which],
                       reinterpret_cast<const T *>(cs->d_coeff[which]), cs->nnz[which], d_asg, d_out, ctx->N, ctx->L, mode,
                       (unsigned)cs->n_inputs, CtxArith<M>::qmod(ctx), cs->d_pidx[which], reinterpret_cast<const T *>(cs->d_ptab));
  });
  RS_HIP(hipGetLastError());
}

constexpr size_t IO_SHORTCUT_MAX_INPUTS = 64;
// does the witness map of this system compute the io vectors as linear forms of the primary inputs (cs->d_io_* hold them
// after the first witness_run)?
// The shortcut needs slot-constant coefficients on the constant one and on the primary inputs (the L_k are slot constant).
bool witness_io_shortcut(const rs_r1cs *cs) { return cs->n_inputs <= IO_SHORTCUT_MAX_INPUTS && !cs->io_poly; }

// Per-circuit cache for the io shortcut: L_k = interp(column k of X), k = 0 (constant) .. n_inputs.
template <class M_>
static void build_io_cache(rs_ctx *ctx, const rs_r1cs *cs, const WitnessPlan *P, const ColPlansT<M_> &cp, hipStream_t st) {
  using T = typename ArithOf<M_>::T;
  if (cs->io_built) return;
  const size_t m = cs->m, M = P->M, L = (size_t)ctx->L;
  std::vector<T> cols;  // [ncols][L][M] data values
  std::vector<int> hk[3], hc[3];
  int ncols = 0;
  for (int w = 0; w < 3; w++) {
    const size_t z = cs->nnz[w];
    for (size_t k = 0; k <= cs->n_inputs; k++) {
      std::vector<uint64_t> y(L * m, 0);
      bool any = false;
      for (size_t r = 0; r < m; r++)
        for (uint32_t e = cs->h_row_ptr[w][r]; e < cs->h_row_ptr[w][r + 1]; e++)
          if (cs->h_col[w][e] == k)
            for (size_t i = 0; i < L; i++) {
              const uint64_t c = cs->h_coeff[w][i * z + e] % ctx->q[i];
              y[i * m + r] = host::addmod(y[i * m + r], c, ctx->q[i]);
              any = any || c != 0;
            }
      if (!any) continue;
      cols.resize((size_t)(ncols + 1) * L * M, T(0));
      for (size_t i = 0; i < L; i++)
        for (size_t r = 0; r < m; r++) cols[((size_t)ncols * L + i) * M + r] = HostArith<M_>::plain(y[i * m + r], ctx->q[i]);
      hk[w].push_back((int)k);
      hc[w].push_back(ncols);
      ncols++;
    }
  }
  rs_r1cs *mc = const_cast<rs_r1cs *>(cs);
  RS_HIP(hipMalloc(&mc->d_io_cols, std::max<size_t>(1, cols.size()) * sizeof(double)));
  if (ncols) {
    RS_HIP(hipMemcpy(mc->d_io_cols, cols.data(), cols.size() * sizeof(double), hipMemcpyHostToDevice));
    launch_interp<M_>(ctx, P, cp, reinterpret_cast<T *>(mc->d_io_cols), (size_t)ncols * L, L, 1, 0, st);
    RS_HIP(hipStreamSynchronize(st));
  }
  for (int w = 0; w < 3; w++) {
    mc->io_count[w] = (int)hk[w].size();
    mc->io_const_col[w] = -1;
    for (size_t c = 0; c < hk[w].size(); c++)
      if (hk[w][c] == 0) mc->io_const_col[w] = hc[w][c];
    const size_t n = std::max<size_t>(1, hk[w].size());
    RS_HIP(hipMalloc(&mc->d_io_k[w], n * sizeof(int)));
    RS_HIP(hipMalloc(&mc->d_io_c[w], n * sizeof(int)));
    if (!hk[w].empty()) {
      RS_HIP(hipMemcpy(mc->d_io_k[w], hk[w].data(), hk[w].size() * sizeof(int), hipMemcpyHostToDevice));
      RS_HIP(hipMemcpy(mc->d_io_c[w], hc[w].data(), hc[w].size() * sizeof(int), hipMemcpyHostToDevice));
    }
  }
  mc->io_M = M;
  mc->io_built = true;
}

// One chunk of the witness map: limbs [limb0, limb0 + nl), slots [cm.slot0, cm.slot0 + cm.ns) of each.
template <class M_>
static void witness_chunk(rs_ctx *ctx, const rs_r1cs *cs, WitnessPlan *P, const uint64_t *d_asg, const uint64_t *d1,
                          const uint64_t *d2, const uint64_t *d3, uint64_t *const outs[7], const ColMap &cm, int nl,
                          const void *d_const_, hipStream_t st, const size_t (*rows)[2]) {
  using T = typename ArithOf<M_>::T;
  using CPS = ColPlansT<M_>;
  const T *d_const = static_cast<const T *>(d_const_);
  const T *io_cols = reinterpret_cast<const T *>(cs->d_io_cols);
  const T *coeff[3] = {reinterpret_cast<const T *>(cs->d_coeff[0]), reinterpret_cast<const T *>(cs->d_coeff[1]),
                       reinterpret_cast<const T *>(cs->d_coeff[2])};
  const M_ *qmod = CtxArith<M_>::qmod(ctx);
  const size_t m = cs->m, M = P->M;
  const size_t C = (size_t)nl * cm.ns;  // columns in this chunk
  const CPS cp = make_colplans<M_>(ctx, P, cm.limb0);
  const bool needH = outs[6] != nullptr;
  const bool shortcut = witness_io_shortcut(cs);
  bool need_io[3], need_full[3], need_cst[3];
  for (int w = 0; w < 3; w++) {
    need_io[w] = outs[w] != nullptr || outs[3 + w] != nullptr;
    need_full[w] = outs[3 + w] != nullptr || (needH && w < 2);  // H needs A and B only
    // a constant part that differs per slot (polynomial coefficients on the constant one) is evaluated and
    // interpolated column by column like the other vectors; the shortcut never sees such a system
    need_cst[w] = cs->const_poly[w] && outs[3 + w] != nullptr;
  }
  // column-major workspace, only the vectors this call needs: io (fallback path only), full, per-slot constant parts, H
  auto needed = [&](int k) {
    return k < 3 ? (need_io[k] && !shortcut) : (k < 6 ? need_full[k - 3] : (k == 6 ? needH : need_cst[k - 7]));
  };
  static const int order[10] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 6};  // the interpolated vectors adjacent, H last
  int slot_of[10], nvec = 0;
  for (int k = 0; k < 10; k++) slot_of[k] = -1;
  for (int o = 0; o < 10; o++)
    if (needed(order[o])) slot_of[order[o]] = nvec++;
  const size_t vec = C * M;
  T *colbuf = (T *)ws_get(ctx, WS_COLUMNS, std::max<size_t>(1, (size_t)nvec * vec) * sizeof(T));
  auto colv = [&](int k) { return colbuf + (size_t)slot_of[k] * vec; };
  RS_REQUIRE((C % 2) == 0 && (M % 2) == 0, "column tiles move slot pairs and row pairs");
  const dim3 tgrid((unsigned)((C + 63) / 64), (unsigned)((M + 63) / 64));    // transposing kernels: 64 x 64 tiles
  const dim3 tgrid_ev((unsigned)((C + 63) / 64), (unsigned)((M + 31) / 32));  // the evaluation: 64 columns x 32 rows
  const T *ptab = reinterpret_cast<const T *>(cs->d_ptab);
  // the map of output vector k: its row range (rows == null: every row)
  auto cm_for = [&](int k) {
    ColMap c = cm;
    if (rows) {
      c.row0 = rows[k][0];
      c.row1 = rows[k][1];
    }
    return c;
  };
  for (int w = 0; w < 3; w++)
    for (int kind = 0; kind < 3; kind++) {  // io, full, constant part
      const int k = kind == 2 ? 7 + w : 3 * kind + w;
      if (!needed(k)) continue;
      // per (row, slot): 8 bytes of assignment per non-zero + 8 bytes of column written
      ProfScope prof(ctx, st, "r1cs_eval_cols_kernel", (double)C * 8.0 * ((double)cs->nnz[w] + (double)M), 7.0 * (double)C * (double)cs->nnz[w]);
      hipLaunchKernelGGL(r1cs_eval_cols_kernel<M_>, tgrid_ev, dim3(256), 0, st, cs->d_row_ptr[w], cs->d_col[w], coeff[w],
                         cs->nnz[w], d_asg, colv(k), m, C, M, kind == 2 ? (int)RS_EVAL_CONST : (kind ? (int)RS_EVAL_FULL : (int)RS_EVAL_IO),
                         (unsigned)cs->n_inputs, qmod, cm, cs->d_pidx[w], ptab);
    }
  RS_HIP(hipGetLastError());
  // one batched interpolation: the needed io / full / constant vectors are adjacent in the workspace
  {
    int n9 = 0;
    for (int k = 0; k < 10; k++) n9 += (k != 6) && needed(k);
    if (n9) launch_interp<M_>(ctx, P, cp, colbuf, (size_t)n9 * C, C, (size_t)cm.ns, cm.limb0, st);
  }
  if (needH) launch_h<M_>(ctx, P, cp, colv(3), colv(4), colv(6), C, (size_t)cm.ns, d1, d2, d3, cm, st, need_full[2] ? colv(5) : (const T *)nullptr);
  const unsigned eb = (unsigned)std::min<size_t>((vec + 255) / 256, 256 * 16);
  if (!shortcut) {
    // fallback: X_mid = interp(full) - interp(io) + interp(constant part), combined in column-major form
    for (int w = 0; w < 3; w++) {
      if (!outs[3 + w]) continue;
      // the constant part: slot constant (interpolated once per call), or per slot when polynomial coefficients
      // multiply the constant one (then the column holds EVERY index-0 term, scalar ones included)
      const T *cst = (!need_cst[w] && d_const && cs->has_const[w]) ? d_const + (size_t)w * ctx->L * M : nullptr;
      ProfScope prof(ctx, st, "mid_kernel", (double)vec * 24.0, 3.0 * (double)vec);
      hipLaunchKernelGGL(mid_kernel<CPS>, dim3(eb), dim3(256), 0, st, colv(3 + w), colv(w), cst, M, C, (unsigned)cm.ns, cp, cm.limb0,
                         need_cst[w] ? colv(7 + w) : (const T *)nullptr);
    }
    RS_HIP(hipGetLastError());
    for (int k = 0; k < 6; k++)
      if (outs[k]) {
        ProfScope prof(ctx, st, "transpose_out_kernel", (double)C * (double)m * 16.0, 0.0);
        hipLaunchKernelGGL(transpose_out_kernel<T>, tgrid, dim3(256), 0, st, colv(k), outs[k], m, C, M, cm_for(k));
      }
  } else {
    for (int w = 0; w < 3; w++) {
      if (!need_io[w]) continue;
      IoDesc io{cs->d_io_k[w], cs->d_io_c[w], cs->io_count[w]};
      if (outs[3 + w]) {  // io (if wanted) and mid in one pass over the interpolated columns
        const T *cst = cs->io_const_col[w] >= 0 ? io_cols + (size_t)cs->io_const_col[w] * ctx->L * M : nullptr;
        // 8 bytes of column read, 8 or 16 written, the primary inputs re-read per row (L2 resident)
        ProfScope prof(ctx, st, "io_mid_out_kernel", (double)C * (double)m * (outs[w] ? 24.0 : 16.0),
                       (double)C * (double)m * (7.0 * io.count + 4.0));
        hipLaunchKernelGGL(io_mid_out_kernel<M_>, tgrid, dim3(256), 0, st, colv(3 + w), io, io_cols, d_asg, cst, outs[w],
                           outs[3 + w], m, C, M, qmod, cm_for(3 + w));  // io and mid of one matrix share their row range (checked by the caller)
      } else {  // io alone: no column work at all
        const unsigned by = (unsigned)((C / 2 + 255) / 256);
        const ColMap cw = cm_for(w);
        const size_t r1 = std::min(m, cw.row1);
        if (r1 <= cw.row0) continue;
        ProfScope prof(ctx, st, "io_coeff_kernel", (double)C * (double)(r1 - cw.row0) * 8.0, (double)C * (double)(r1 - cw.row0) * 7.0 * io.count);
        hipLaunchKernelGGL(io_coeff_kernel<M_>, dim3((unsigned)(r1 - cw.row0), by), dim3(256), 0, st, io, io_cols, d_asg, outs[w], C, M, qmod, cw);
      }
    }
  }
  RS_HIP(hipGetLastError());
  if (needH) {
    {
      ProfScope prof(ctx, st, "transpose_out_kernel", (double)C * (double)m * 16.0, 0.0);
      hipLaunchKernelGGL(transpose_out_kernel<T>, tgrid, dim3(256), 0, st, colv(6), outs[6], std::min(m + 1, M), C, M, cm_for(6));
    }
    const ColMap ch = cm_for(6);
    if (m == M && m >= ch.row0 && m < ch.row1)  // row m does not exist in the M-row column tile
      hipLaunchKernelGGL(h_top_kernel<M_>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, outs[6] + (m - ch.row0) * cm.out_stride(), d1, d2, C,
                         qmod, cm);
    RS_HIP(hipGetLastError());
  }
}

// Witness map driver.  outs[k] (k = A_io,B_io,C_io,A_mid,B_mid,C_mid,H) may be null.  Slots
// [slot0, slot0 + nslots) of every limb are processed; `compact` selects the output layout
// [t][L][nslots] (a slot-sharded rank) instead of the full [t][L][N].  The columns are
// worked through in chunks whose column-major workspace stays within g_tune.witness_col_budget_mib
// (at m = 2^16 and the headline ring that is one limb at a time: 3 x 4 GiB instead of 7 x 16 GiB).
template <class M_>
static void witness_run_arith(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_asg, const uint64_t *d1, const uint64_t *d2,
                              const uint64_t *d3, uint64_t *const outs[7], uint64_t *h_Z, hipStream_t st, int slot0, int nslots,
                              bool compact, const size_t (*rows)[2]) {
  using T = typename ArithOf<M_>::T;
  RS_REQUIRE((d1 && d2 && d3) || (!d1 && !d2 && !d3), "d1,d2,d3 must be all set or all null");
  if (nslots < 0) nslots = ctx->N - slot0;
  RS_REQUIRE(slot0 >= 0 && nslots >= 2 && slot0 + nslots <= ctx->N && !(slot0 & 1) && !(nslots & 1),
             "slot range must be even-aligned and inside the ring");
  const size_t m = cs->m;
  if (rows) {
    for (int k = 0; k < 7; k++)
      RS_REQUIRE(!outs[k] || (rows[k][0] <= rows[k][1] && rows[k][1] <= m + (k == 6 ? 1 : 0)), "row range outside the vector");
    for (int w = 0; w < 3; w++)
      RS_REQUIRE(!outs[w] || !outs[3 + w] || (rows[w][0] == rows[3 + w][0] && rows[w][1] == rows[3 + w][1]),
                 "the io and mid vectors of one matrix take the same row range");
  }
  WitnessPlan *P = get_plan(ctx, m);
  const size_t M = P->M;
  const int L = ctx->L;
  if (h_Z)
    for (int i = 0; i < L; i++) memcpy(h_Z + (size_t)i * (m + 1), P->limb[i].Z.data(), sizeof(uint64_t) * (m + 1));
  const bool shortcut = witness_io_shortcut(cs);
  if (shortcut) build_io_cache<M_>(ctx, cs, P, make_colplans<M_>(ctx, P), st);
  // fallback path: interpolated constant parts [3][L][M], once per call
  T *d_const = nullptr;
  if (!shortcut && (cs->has_const[0] || cs->has_const[1] || cs->has_const[2]) && (outs[3] || outs[4] || outs[5])) {
    std::vector<T> hc((size_t)3 * L * M, T(0));
    for (int w = 0; w < 3; w++)
      for (int i = 0; i < L; i++)
        for (size_t r = 0; r < m; r++) hc[((size_t)w * L + i) * M + r] = HostArith<M_>::plain(cs->h_const[w][(size_t)i * m + r], ctx->q[i]);
    d_const = (T *)ws_get(ctx, WS_SIDE, hc.size() * sizeof(T));
    RS_HIP(hipMemcpyAsync(d_const, hc.data(), hc.size() * sizeof(T), hipMemcpyHostToDevice, st));
    RS_HIP(hipStreamSynchronize(st));  // hc goes out of scope
    launch_interp<M_>(ctx, P, make_colplans<M_>(ctx, P), d_const, (size_t)3 * L, (size_t)L, 1, 0, st);
  }
  // chunking: as many whole limbs as fit the budget, else pieces of one limb (multiples of 64 slots)
  int nvec = 0;
  {
    const bool needH = outs[6] != nullptr;
    for (int w = 0; w < 3; w++) {
      const bool need_io = outs[w] || outs[3 + w], need_full = outs[3 + w] || (needH && w < 2);
      nvec += (need_io && !shortcut) + need_full + (cs->const_poly[w] && outs[3 + w]);
    }
    nvec += needH;
  }
  const size_t budget_cols =
      std::max<size_t>(64, ((size_t)g_tune.witness_col_budget_mib << 20) / (std::max(1, nvec) * M * sizeof(double)));
  ColMap cm{0, nslots, slot0, ctx->N, L, compact ? nslots : ctx->N, compact ? slot0 : 0};
  if ((size_t)nslots <= budget_cols) {
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)L, budget_cols / (size_t)nslots));
    for (int l0 = 0; l0 < L; l0 += per) {
      cm.limb0 = l0;
      witness_chunk<M_>(ctx, cs, P, d_asg, d1, d2, d3, outs, cm, std::min(per, L - l0), d_const, st, rows);
    }
  } else {
    const int piece = (int)std::max<size_t>(64, (budget_cols / 64) * 64);
    for (int l0 = 0; l0 < L; l0++)
      for (int s0 = 0; s0 < nslots; s0 += piece) {
        cm.limb0 = l0;
        cm.slot0 = slot0 + s0;
        cm.ns = std::min(piece, nslots - s0);
        witness_chunk<M_>(ctx, cs, P, d_asg, d1, d2, d3, outs, cm, 1, d_const, st, rows);
      }
  }
}
void witness_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_asg, const uint64_t *d1, const uint64_t *d2,
                 const uint64_t *d3, uint64_t *const outs[7], uint64_t *h_Z, hipStream_t st, int slot0, int nslots, bool compact,
                 const size_t (*rows)[2]) {
  dispatch_arith(ctx, [&](auto tag) { witness_run_arith<decltype(tag)>(ctx, cs, d_asg, d1, d2, d3, outs, h_Z, st, slot0, nslots, compact, rows); });
}

template <class M_>
static void interpolate_arith(rs_ctx *ctx, const uint64_t *d_y, uint64_t *d_out, size_t n, hipStream_t st) {
  using T = typename ArithOf<M_>::T;
  WitnessPlan *P = get_plan(ctx, n);
  const ColPlansT<M_> cp = make_colplans<M_>(ctx, P);
  const size_t M = P->M, S_ = ctx->ring_words();
  T *colbuf = (T *)ws_get(ctx, WS_COLUMNS, S_ * M * sizeof(T));
  const dim3 tgrid((unsigned)((S_ + 31) / 32), (unsigned)((M + 31) / 32));
  const ColMap cm{0, ctx->N, 0, ctx->N, ctx->L, ctx->N, 0};
  hipLaunchKernelGGL(transpose_in_kernel<T>, tgrid, dim3(256), 0, st, d_y, colbuf, n, S_, M);
  launch_interp<M_>(ctx, P, cp, colbuf, S_, S_, (size_t)ctx->N, 0, st);
  const dim3 ogrid((unsigned)((S_ + 63) / 64), (unsigned)((M + 63) / 64));
  hipLaunchKernelGGL(transpose_out_kernel<T>, ogrid, dim3(256), 0, st, colbuf, d_out, n, S_, M, cm);
  RS_HIP(hipGetLastError());
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_r1cs_create(rs_ctx *ctx, size_t m, size_t n_vars, size_t n_inputs, const uint32_t *const h_row_ptr[3],
                   const uint32_t *const h_col[3], const uint64_t *const h_coeff[3], const size_t nnz[3], rs_r1cs **out) {
  return rs_r1cs_create_poly(ctx, m, n_vars, n_inputs, h_row_ptr, h_col, h_coeff, nnz, nullptr, nullptr, 0, out);
}

int rs_r1cs_create_poly(rs_ctx *ctx, size_t m, size_t n_vars, size_t n_inputs, const uint32_t *const h_row_ptr[3],
                        const uint32_t *const h_col[3], const uint64_t *const h_coeff[3], const size_t nnz[3],
                        const int32_t *const h_poly_idx[3], const uint64_t *h_poly_table, size_t n_poly, rs_r1cs **out) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && out && h_row_ptr && h_col && h_coeff && nnz, "null argument");
  RS_REQUIRE(m >= 1 && n_inputs <= n_vars, "bad R1CS shape");
  RS_REQUIRE(n_poly == 0 || (h_poly_idx && h_poly_table), "polynomial coefficient table without indices");
  struct Holder {  // frees a partly built object when a check below throws
    rs_r1cs *p;
    ~Holder() { rs_r1cs_destroy(p); }
  } holder{new rs_r1cs()};
  rs_r1cs *cs = holder.p;
  cs->m = m;
  cs->n_vars = n_vars;
  cs->n_inputs = n_inputs;
  cs->L = ctx->L;
  cs->n_poly = n_poly;
  const size_t rw = ctx->ring_words();
  if (n_poly) {  // the table as constants of the context's arithmetic, in the ring layout [n_poly][L][N]
    cs->h_ptab.assign(h_poly_table, h_poly_table + n_poly * rw);
    std::vector<uint64_t> pt(n_poly * rw);
    for (size_t k = 0; k < n_poly; k++)
      for (int i = 0; i < ctx->L; i++)
        for (int x = 0; x < ctx->N; x++) {
          const size_t at = (k * ctx->L + i) * (size_t)ctx->N + x;
          cs->h_ptab[at] %= ctx->q[i];
          pt[at] = konst_word(ctx, cs->h_ptab[at], ctx->q[i]);
        }
    RS_HIP(hipMalloc(&cs->d_ptab, sizeof(double) * pt.size()));
    RS_HIP(hipMemcpy(cs->d_ptab, pt.data(), sizeof(double) * pt.size(), hipMemcpyHostToDevice));
  }
  for (int w = 0; w < 3; w++) {
    const size_t z = nnz[w];
    cs->nnz[w] = z;
    RS_REQUIRE(h_row_ptr[w] && (h_col[w] || z == 0) && (h_coeff[w] || z == 0), "null matrix array");
    RS_REQUIRE(h_row_ptr[w][0] == 0 && h_row_ptr[w][m] == z, "row_ptr does not match nnz");
    for (size_t r = 0; r < m; r++) RS_REQUIRE(h_row_ptr[w][r] <= h_row_ptr[w][r + 1], "row_ptr is not monotone");
    cs->h_row_ptr[w].assign(h_row_ptr[w], h_row_ptr[w] + m + 1);
    cs->h_col[w].assign(h_col[w], h_col[w] + z);
    cs->h_coeff[w].assign(h_coeff[w], h_coeff[w] + (size_t)ctx->L * z);
    cs->h_const[w].assign((size_t)ctx->L * m, 0);
    cs->has_const[w] = false;
    const int32_t *pidx = (n_poly && h_poly_idx[w]) ? h_poly_idx[w] : nullptr;
    bool any_poly = false;
    for (size_t e = 0; pidx && e < z; e++) {
      RS_REQUIRE(pidx[e] < 0 || (size_t)pidx[e] < n_poly, "polynomial coefficient index out of range");
      if (pidx[e] < 0) continue;
      any_poly = true;
      if (h_col[w][e] <= n_inputs) cs->io_poly = true;
      if (h_col[w][e] == 0) cs->const_poly[w] = true;
    }
    std::vector<uint64_t> cf((size_t)ctx->L * std::max<size_t>(z, 1), 0);  // table constants of the context's arithmetic
    for (size_t r = 0; r < m; r++)
      for (uint32_t e = h_row_ptr[w][r]; e < h_row_ptr[w][r + 1]; e++) {
        RS_REQUIRE(h_col[w][e] <= n_vars, "column index out of range");
        const bool is_poly = pidx && pidx[e] >= 0;
        for (int i = 0; i < ctx->L; i++) {
          const uint64_t c = is_poly ? 0 : h_coeff[w][(size_t)i * z + e] % ctx->q[i];  // the scalar slot of a polynomial term is unused
          cs->h_coeff[w][(size_t)i * z + e] = c;
          cf[(size_t)i * z + e] = konst_word(ctx, c, ctx->q[i]);
          if (h_col[w][e] == 0) {
            cs->h_const[w][(size_t)i * m + r] = host::addmod(cs->h_const[w][(size_t)i * m + r], c, ctx->q[i]);
            if (c) cs->has_const[w] = true;
          }
        }
      }
    RS_HIP(hipMalloc(&cs->d_row_ptr[w], sizeof(uint32_t) * (m + 1)));
    RS_HIP(hipMemcpy(cs->d_row_ptr[w], h_row_ptr[w], sizeof(uint32_t) * (m + 1), hipMemcpyHostToDevice));
    RS_HIP(hipMalloc(&cs->d_col[w], sizeof(uint32_t) * std::max<size_t>(z, 1)));
    if (z) RS_HIP(hipMemcpy(cs->d_col[w], h_col[w], sizeof(uint32_t) * z, hipMemcpyHostToDevice));
    RS_HIP(hipMalloc(&cs->d_coeff[w], sizeof(double) * cf.size()));
    RS_HIP(hipMemcpy(cs->d_coeff[w], cf.data(), sizeof(double) * cf.size(), hipMemcpyHostToDevice));
    if (any_poly) {
      cs->h_pidx[w].assign(pidx, pidx + z);
      RS_HIP(hipMalloc(&cs->d_pidx[w], sizeof(int32_t) * z));
      RS_HIP(hipMemcpy(cs->d_pidx[w], pidx, sizeof(int32_t) * z, hipMemcpyHostToDevice));
    }
  }
  holder.p = nullptr;
  *out = cs;
  RS_API_END
}

void rs_r1cs_destroy(rs_r1cs *cs) {
  if (!cs) return;
  for (int w = 0; w < 3; w++) {
    if (cs->d_row_ptr[w]) (void)hipFree(cs->d_row_ptr[w]);
    if (cs->d_col[w]) (void)hipFree(cs->d_col[w]);
    if (cs->d_coeff[w]) (void)hipFree(cs->d_coeff[w]);
    if (cs->d_io_k[w]) (void)hipFree(cs->d_io_k[w]);
    if (cs->d_io_c[w]) (void)hipFree(cs->d_io_c[w]);
    if (cs->d_pidx[w]) (void)hipFree(cs->d_pidx[w]);
  }
  if (cs->d_io_cols) (void)hipFree(cs->d_io_cols);
  if (cs->d_ptab) (void)hipFree(cs->d_ptab);
  delete cs;
}

int rs_r1cs_evaluate(rs_ctx *ctx, const rs_r1cs *cs, int which, int mode, const uint64_t *d_assignment, uint64_t *d_out,
                     rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && cs && d_assignment && d_out, "null argument");
  RS_REQUIRE(which >= 0 && which < 3 && mode >= 0 && mode <= 2, "bad selector");
  r1cs_evaluate_run(ctx, cs, which, mode, d_assignment, d_out, S(stream));
  RS_API_END
}

int rs_witness_map(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_assignment, const uint64_t *d_d1,
                   const uint64_t *d_d2, const uint64_t *d_d3, uint64_t *d_A_io, uint64_t *d_B_io, uint64_t *d_C_io,
                   uint64_t *d_A_mid, uint64_t *d_B_mid, uint64_t *d_C_mid, uint64_t *d_H, uint64_t *h_Z,
                   rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && cs && d_assignment, "null argument");
  WsScope ws_scope(ctx, S(stream));
  uint64_t *outs[7] = {d_A_io, d_B_io, d_C_io, d_A_mid, d_B_mid, d_C_mid, d_H};
  witness_run(ctx, cs, d_assignment, d_d1, d_d2, d_d3, outs, h_Z, S(stream));
  RS_API_END
}

int rs_witness_map_slots(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_assignment, const uint64_t *d_d1,
                         const uint64_t *d_d2, const uint64_t *d_d3, int slot0, int nslots, uint64_t *d_A_io,
                         uint64_t *d_B_io, uint64_t *d_C_io, uint64_t *d_A_mid, uint64_t *d_B_mid, uint64_t *d_C_mid,
                         uint64_t *d_H, uint64_t *h_Z, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && cs && d_assignment, "null argument");
  WsScope ws_scope(ctx, S(stream));
  uint64_t *outs[7] = {d_A_io, d_B_io, d_C_io, d_A_mid, d_B_mid, d_C_mid, d_H};
  witness_run(ctx, cs, d_assignment, d_d1, d_d2, d_d3, outs, h_Z, S(stream), slot0, nslots, true);
  RS_API_END
}

int rs_witness_map_rows(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_assignment, const uint64_t *d_d1,
                        const uint64_t *d_d2, const uint64_t *d_d3, const size_t *h_rows, uint64_t *d_A_io, uint64_t *d_B_io,
                        uint64_t *d_C_io, uint64_t *d_A_mid, uint64_t *d_B_mid, uint64_t *d_C_mid, uint64_t *d_H, uint64_t *h_Z,
                        rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && cs && d_assignment && h_rows, "null argument");
  WsScope ws_scope(ctx, S(stream));
  uint64_t *outs[7] = {d_A_io, d_B_io, d_C_io, d_A_mid, d_B_mid, d_C_mid, d_H};
  size_t rows[7][2];
  for (int k = 0; k < 7; k++) rows[k][0] = h_rows[2 * k], rows[k][1] = h_rows[2 * k + 1];
  witness_run(ctx, cs, d_assignment, d_d1, d_d2, d_d3, outs, h_Z, S(stream), 0, -1, false, rows);
  RS_API_END
}

int rs_interpolate(rs_ctx *ctx, const uint64_t *d_y, uint64_t *d_out, size_t n, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_y && d_out && n >= 1, "null argument");
  WsScope ws_scope(ctx, S(stream));
  dispatch_arith(ctx, [&](auto tag) { interpolate_arith<decltype(tag)>(ctx, d_y, d_out, n, S(stream)); });
  RS_API_END
}

}  // extern "C"
