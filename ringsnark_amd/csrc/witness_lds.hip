// witness_lds.hip -- every launch of the witness map whose kernel runs the generic LDS round functions of ntt_core.hpp: the
// product tree's tiles, the columns that fit one LDS tile, the block convolutions, and the generic sub-transform kernel of
// the multi-pass path (witness.hip has the map of the units).
// ONE unit on purpose: these kernels share instantiations of the round functions, and hipcc specialises a device function on
// the callers its unit shows it before it inlines it -- compiled apart, 38 of these kernels come out with other code, some
// with more registers and spills (tools/device_asm_diff.sh).  The sections below are cut by launch path all the same.
#include <algorithm>
#include <type_traits>

#include "witness_bc.hpp"
#include "witness_launch.hpp"
#include "witness_tiles.hpp"
#include "witness_tree_wide.hpp"

namespace rs {

// ---- the product tree's tiles, for every path --------------------------------------------------------------
// Newton -> monomial levels 1..logT on tiles of 2^logT coefficients of [ncols][M] columns; with
// `newton` (logT == logM) the tiles hold values and the Newton conversion runs first, in the same launch
// FP64 instructions (per lane) of the product tree on one tile of T = 2^logT coefficients: levels
// 1..4 by schoolbook (120 modular multiplies + as many additions per 16 coefficients), every level
// above by a forward and an inverse batched transform plus the spectrum product and the recombination
// pw_reduce: the spectrum is reduced before it meets the table entry (3 more instructions per coefficient and level;
// the wide kernel does it only where ColPlan::pwmask asks for it)
double tree_fp64(double T, int logT, bool pw_reduce) {
  double f = T / 16.0 * (120.0 * 7.0 + 4.0 * 16.0 * 3.0);
  for (int l = SCHOOL_LEVELS + 1; l <= logT; l++) f += 2.0 * ntt_fp64(T, l) + (pw_reduce ? 10.0 : 7.0) * T;
  return f;
}
// Wout / rf (2^14 tiles of the wide kernel only): the right tiles also run the rf forward cross stages of level 15 and write
// that level's workspace [ncols][2^logM] (tree_wide_kernel<14, RF>); the caller then skips the level's source pass.
static bool wide_ok_for_fwd(int logT, int rf) { return g_tune.witness_tree_ct == 2 && logT == 14 && (rf == 2 || rf == 3); }
void launch_tree_tiles(rs_ctx *ctx, double *cols, size_t ncols, size_t col0, int logM, int logT, size_t S,
                              size_t slots_per_limb, const ColPlans &cp, hipStream_t st, bool newton, double *Wout, int rf) {
  const size_t T = (size_t)1 << logT;
  const double tiles = (double)(ncols << (logM - logT));
  // Newton conversion (single-tile columns): two passes of forward + inverse M-point transforms and two pointwise products
  const double newton_fp64 = newton ? 4.0 * ntt_fp64((double)T, logT) + 31.0 * (double)T : 0.0;
  // names as rocprofv3 prints them (a prefix of "rs::<name>") so that profiles/ and the live record can be joined
  const bool ct13 = logT == 13 && g_tune.witness_tree_ct;
  const bool wide = !newton && g_tune.witness_tree_ct == 2 && (logT == 13 || logT == 14);
  RS_REQUIRE(!Wout || (wide_ok_for_fwd(logT, rf) && !newton), "tree tiles: forward stages of the next level need the wide 2^14 tile");
  const char *pname = wide ? (logT == 14 ? (Wout ? (rf == 3 ? "tree_wide_kernel<14, 3>" : "tree_wide_kernel<14, 2>") : "tree_wide_kernel<14, 0>") : "tree_wide_kernel<13, 0>")
                      : ct13 ? (newton ? "tree_columns_kernel<512, 13, true>" : "tree_columns_kernel<512, 13, false>")
                           : (newton ? "tree_columns_kernel<NEWTON>" : "tree_columns_kernel");
  bool pw = !wide;  // the model count follows what the wide kernel executes: the pre-product reduction per level only where asked for
  if (wide)
    for (int i = 0; i < RS_MAX_L; i++) pw = pw || ((cp.l[i].pwmask >> logT) & 1u);
  // with Wout: half of the tiles also write a 2^(logT+1)-word node of the next level's workspace, rf - 1 stages each
  ProfScope prof(ctx, st, pname, tiles * (double)T * (Wout ? 24.0 : 16.0),
                 tiles * (tree_fp64((double)T, logT, pw) + newton_fp64) + (Wout ? tiles / 2.0 * ntt_fp64(2.0 * (double)T, rf - 1) : 0.0));
  const size_t lds1 = padded_len(T) * sizeof(double);
  const unsigned grid = (unsigned)(ncols << (logM - logT));
  const int thr = (int)std::max<size_t>(64, std::min<size_t>(1024, T / 16));  // 1024 only for a 2^14 tile (one workgroup per CU)
  RS_REQUIRE(wide || (T / thr <= 16 && logT >= 6), "tree tile out of range");
  RS_REQUIRE(!newton || logT == logM, "fused Newton conversion needs single-tile columns");
#define RS_TREE_LAUNCH_K(KERN)                                                                                   \
  do {                                                                                                           \
    set_max_dyn_lds((const void *)KERN, (int)lds1);     \
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(thr), lds1, st, cols, logM, logT, col0, (unsigned)S,               \
                       (unsigned)slots_per_limb, cp);                                                            \
  } while (0)
#define RS_TREE_LAUNCH(THR)                                          \
  do {                                                               \
    if (newton)                                                      \
      RS_TREE_LAUNCH_K((tree_columns_kernel<THR, 0, true>));         \
    else                                                             \
      RS_TREE_LAUNCH_K((tree_columns_kernel<THR, 0, false>));        \
  } while (0)
  if (wide) {
    const int wl = (int)((T + T / 32) * sizeof(double));
    if (logT == 14 && Wout && rf == 3) {
      set_max_dyn_lds((const void *)tree_wide_kernel<14, 3>, wl);
      hipLaunchKernelGGL((tree_wide_kernel<14, 3>), dim3(grid), dim3(512), wl, st, cols, logM, col0, (unsigned)S, (unsigned)slots_per_limb, cp, Wout);
    } else if (logT == 14 && Wout) {
      set_max_dyn_lds((const void *)tree_wide_kernel<14, 2>, wl);
      hipLaunchKernelGGL((tree_wide_kernel<14, 2>), dim3(grid), dim3(512), wl, st, cols, logM, col0, (unsigned)S, (unsigned)slots_per_limb, cp, Wout);
    } else if (logT == 14) {
      set_max_dyn_lds((const void *)tree_wide_kernel<14, 0>, wl);
      hipLaunchKernelGGL((tree_wide_kernel<14, 0>), dim3(grid), dim3(512), wl, st, cols, logM, col0, (unsigned)S, (unsigned)slots_per_limb, cp,
                         (double *)nullptr);
    } else {
      set_max_dyn_lds((const void *)tree_wide_kernel<13, 0>, wl);
      hipLaunchKernelGGL((tree_wide_kernel<13, 0>), dim3(grid), dim3(256), wl, st, cols, logM, col0, (unsigned)S, (unsigned)slots_per_limb, cp,
                         (double *)nullptr);
    }
  } else if (thr == 512 && logT == 13 && g_tune.witness_tree_ct) {
    if (newton)
      RS_TREE_LAUNCH_K((tree_columns_kernel<512, 13, true>));
    else
      RS_TREE_LAUNCH_K((tree_columns_kernel<512, 13, false>));
  } else if (thr == 1024) RS_TREE_LAUNCH(1024);
  else if (thr == 512) RS_TREE_LAUNCH(512);
  else if (thr == 256) RS_TREE_LAUNCH(256);
  else if (thr == 128) RS_TREE_LAUNCH(128);
  else RS_TREE_LAUNCH(64);
#undef RS_TREE_LAUNCH
#undef RS_TREE_LAUNCH_K
  RS_HIP(hipGetLastError());
}

// The same tile work for any arithmetic (the integer contexts): levels 1..logT of the product tree on tiles of
// 2^logT Newton coefficients, tile + scratch in LDS, all-barrier rounds.
template <class CPS>
__global__ void __launch_bounds__(1024)
tree_tiles_generic_kernel(typename CPS::T *__restrict__ cols, int logM, int logT, size_t col0, unsigned S, unsigned slots_per_limb,
                          CPS plans) {
  using T = typename CPS::T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T *s = reinterpret_cast<T *>(smem);
  const unsigned nb = 1u << (logM - logT);
  const size_t col = blockIdx.x / nb;
  const int pos0 = (int)(blockIdx.x % nb) << logT, Tn = 1 << logT;
  const ColPlanT<typename CPS::M> &P = plans.l[((col0 + col) % S) / slots_per_limb];
  T *c = cols + col * ((size_t)1 << logM) + pos0;
  for (int i = threadIdx.x; i < Tn; i += blockDim.x) s[pidx(i)] = c[i];
  __syncthreads();
  tree_levels_lds(s, logT, logM, pos0, P);
  for (int i = threadIdx.x; i < Tn; i += blockDim.x) c[i] = reduce(s[pidx(i)], P.mod);
}
template <class M>
void launch_tree_tiles_generic(rs_ctx *ctx, typename ArithOf<M>::T *cols, size_t ncols, size_t col0, int logM, int logT, size_t S,
                                      size_t slots_per_limb, const ColPlansT<M> &cp, hipStream_t st) {
  const size_t T = (size_t)1 << logT;
  const size_t lds = padded_len(tree_scratch_offset((int)T) + T) * sizeof(uint64_t);
  ProfScope prof(ctx, st, "tree_tiles_generic_kernel", (double)(ncols << (logM - logT)) * (double)T * 16.0,
                 (double)(ncols << (logM - logT)) * tree_fp64((double)T, logT));
  set_max_dyn_lds((const void *)tree_tiles_generic_kernel<ColPlansT<M>>, (int)lds);
  hipLaunchKernelGGL(tree_tiles_generic_kernel<ColPlansT<M>>, dim3((unsigned)(ncols << (logM - logT))), dim3(col_threads(2 * T)), lds, st,
                     cols, logM, logT, col0, (unsigned)S, (unsigned)slots_per_limb, cp);
  RS_HIP(hipGetLastError());
}
#define RS_INSTANTIATE(M) \
  template void launch_tree_tiles_generic<M>(rs_ctx *, ArithOf<M>::T *, size_t, size_t, int, int, size_t, size_t, const ColPlansT<M> &, hipStream_t);
RS_INSTANTIATE(Mod)
RS_INSTANTIATE(ModI)
#undef RS_INSTANTIATE

// ---- a whole column in one LDS tile: interpolation and H of small columns, H of the single-tile columns ------
int col_threads(size_t M) { return (int)std::max<size_t>(64, std::min<size_t>(1024, M / 8)); }

template <class M>
void launch_interp_columns(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *cols, size_t ncols, size_t S,
                           size_t slots_per_limb, hipStream_t st) {
  // the 2M convolution tile, or the product tree's tile + scratch when M is below the LDS block size
  const size_t lds = std::max(padded_len(2 * P->M), padded_len(tree_scratch_offset((int)P->M) + P->M)) * sizeof(double);
  set_max_dyn_lds((const void *)interp_columns_kernel<ColPlansT<M>>, (int)lds);
  ProfScope prof(ctx, st, "interp_columns_kernel", (double)ncols * (double)P->M * 16.0,
                 (double)ncols * (2.0 * ntt_fp64(2.0 * (double)P->M, P->logM + 1) + 21.0 * (double)P->M + tree_fp64((double)P->M, P->logM)));
  hipLaunchKernelGGL(interp_columns_kernel<ColPlansT<M>>, dim3((unsigned)ncols), dim3(col_threads(2 * P->M)), lds, st, cols, P->logM,
                     (unsigned)S, (unsigned)slots_per_limb, cp);
  RS_HIP(hipGetLastError());
}

void launch_h_tile(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, const double *A, const double *B, double *H, size_t S, size_t spl,
                   const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, hipStream_t st) {
  const size_t Mlen = P->M;
  const size_t lds1 = padded_len(Mlen) * sizeof(double);
  const int thr = (int)(Mlen / 16);
  // ten M-point transforms, four pointwise products, the ZK patch
  ProfScope prof(ctx, st, "h_tile_kernel", (double)S * (double)Mlen * 24.0,
                 (double)S * (10.0 * ntt_fp64((double)Mlen, P->logM) + (d1 ? 52.0 : 28.0) * (double)Mlen));
#define RS_H_LAUNCH(KERN)                                                                                            \
  do {                                                                                                               \
    set_max_dyn_lds((const void *)KERN, (int)lds1);         \
    hipLaunchKernelGGL(KERN, dim3((unsigned)S), dim3(thr), lds1, st, A, B, H, P->logM, (int)P->m, (unsigned)spl, cp, \
                       d1, d2, d3, cm);                                                                              \
  } while (0)
  if (thr == 1024) RS_H_LAUNCH((h_tile_kernel<1024, 0>));
  else if (thr == 512 && g_tune.witness_tree_ct) RS_H_LAUNCH((h_tile_kernel<512, 13>));
  else if (thr == 512) RS_H_LAUNCH((h_tile_kernel<512, 0>));
  else if (thr == 256) RS_H_LAUNCH((h_tile_kernel<256, 0>));
  else if (thr == 128) RS_H_LAUNCH((h_tile_kernel<128, 0>));
  else RS_H_LAUNCH((h_tile_kernel<64, 0>));
#undef RS_H_LAUNCH
  RS_HIP(hipGetLastError());
}

template <class M>
void launch_h_columns(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A,
                      const typename ArithOf<M>::T *B, typename ArithOf<M>::T *H, size_t S, size_t spl, const uint64_t *d1,
                      const uint64_t *d2, const uint64_t *d3, const ColMap &cm, hipStream_t st) {
  const size_t Mlen = P->M;
  const size_t lds = padded_len(2 * Mlen) * sizeof(double);
  set_max_dyn_lds((const void *)h_columns_kernel<ColPlansT<M>>, (int)lds);
  ProfScope prof(ctx, st, "h_columns_kernel", (double)S * (double)Mlen * 24.0,
                 (double)S * (5.0 * ntt_fp64(2.0 * (double)Mlen, P->logM + 1) + (d1 ? 52.0 : 28.0) * (double)Mlen));
  hipLaunchKernelGGL(h_columns_kernel<ColPlansT<M>>, dim3((unsigned)S), dim3(col_threads(2 * Mlen)), lds, st, A, B, H, P->logM, (int)P->m,
                     (unsigned)spl, cp, d1, d2, d3, cm);
  RS_HIP(hipGetLastError());
}

#define RS_INSTANTIATE(M)                                                                                                                    \
  template void launch_interp_columns<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, ArithOf<M>::T *, size_t, size_t, size_t, hipStream_t); \
  template void launch_h_columns<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, const ArithOf<M>::T *, const ArithOf<M>::T *,         \
                                    ArithOf<M>::T *, size_t, size_t, const uint64_t *, const uint64_t *, const uint64_t *, const ColMap &,   \
                                    hipStream_t);
RS_INSTANTIATE(Mod)
RS_INSTANTIATE(ModI)
#undef RS_INSTANTIATE

// ---- block-convolution path: host side ---------------------------------------------------------------------
template <int SRC, int YK, int DST, class M>
static void bc_conv(rs_ctx *ctx, BcArgs a, size_t ncols, size_t per_unit, const ColPlansT<M> &cp, hipStream_t st) {
  using CPS = ColPlansT<M>;
  const size_t B2 = (size_t)1 << a.bcLog, lds = padded_len(B2) * sizeof(uint64_t);
  const int thr = col_threads(B2);
  const double nfwd = (double)ncols * a.units * a.nxb, nmac = (double)ncols * a.units * a.nk;
  double pairs = 0;  // pointwise block products
  for (int k = 0; k < a.nk; k++) pairs += std::min(k, a.nxb - 1) - std::max(0, k - a.nyb + 1) + 1;
  {
    ProfScope prof(ctx, st, "bc_fwd_kernel", nfwd * (double)B2 * 12.0, nfwd * ntt_fp64((double)B2, a.bcLog));
    set_max_dyn_lds((const void *)bc_fwd_kernel<SRC, CPS>, (int)lds);
    hipLaunchKernelGGL((bc_fwd_kernel<SRC, CPS>), dim3((unsigned)(ncols * a.units * a.nxb)), dim3(thr), lds, st, a, cp);
  }
  {
    ProfScope prof(ctx, st, "bc_mac_kernel", nmac * (double)B2 * 8.0 + (double)ncols * a.units * pairs * (double)B2 * 8.0,
                   nmac * ntt_fp64((double)B2, a.bcLog) + (double)ncols * a.units * pairs * (double)B2 * 7.0);
    set_max_dyn_lds((const void *)bc_mac_kernel<YK, CPS>, (int)lds);
    hipLaunchKernelGGL((bc_mac_kernel<YK, CPS>), dim3((unsigned)(ncols * a.units * a.nk)), dim3(thr), lds, st, a, cp);
  }
  {
    const size_t total = ncols * a.units * per_unit;
    ProfScope prof(ctx, st, "bc_out_kernel", (double)total * 24.0, (double)total * 3.0);
    hipLaunchKernelGGL((bc_out_kernel<DST, CPS>), dim3((unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, 256 * 32))), dim3(256), 0,
                       st, a, cp, ncols, per_unit);
  }
  RS_HIP(hipGetLastError());
}

// columns per chunk such that the block workspaces (spectra + pair products, up to ~8M words per column) stay within ~6 GiB
size_t bc_chunk_cols(const WitnessPlan *P) {
  return std::max<size_t>(1, ((size_t)g_tune.witness_big_ws_mib << 20) / ((P->bc2 ? 12 : 10) * P->M * sizeof(double)));
}

template <class M>
void bc_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *X, size_t ncols, size_t col0,
                      size_t S, size_t spl, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const int logM = P->logM, bc = P->bcLog;
  const size_t Mlen = P->M, B = (size_t)1 << (bc - 1);
  T *Xhat = (T *)ws_get(ctx, WS_PASS_A, ncols * 2 * Mlen * sizeof(T));
  T *Wc = (T *)ws_get(ctx, WS_PASS_B, ncols * 2 * Mlen * sizeof(T));
  BcArgs a{};
  a.src = X;
  a.dst = X;
  a.Xhat = Xhat;
  a.Wc = Wc;
  a.bcLog = bc;
  a.logM = logM;
  a.m = (int)P->m;
  a.col0 = col0;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  // values -> Newton coefficients: low M terms of (y_k / k!) * ((-1)^k / k!)
  a.units = 1;
  a.nxb = a.nyb = a.nk = (int)(Mlen / B);
  bc_conv<BS_SCALE, BY_E, BD_NEWTON, M>(ctx, a, ncols, Mlen, cp, st);
  // product tree: levels <= bc inside LDS tiles (transforms of length <= 2^bc) ...
  if constexpr (std::is_same<M, Mod>::value) {
    // ... through the wide tile kernel where it exists (2^13 / 2^14 tiles: the recipe primes of the headline shape have
    // 2-adicity 14, so the whole 2^14 tile of tree_wide_kernel<14> is available to them)
    if ((bc == 13 || bc == 14) && g_tune.witness_tree_ct == 2 && (bc == 13 || g_tune.witness_tree_log >= 14))
      launch_tree_tiles(ctx, X, ncols, col0, logM, bc, S, spl, cp, st);
    else
      launch_tree_tiles_generic<M>(ctx, X, ncols, col0, logM, bc, S, spl, cp, st);
  } else {
    launch_tree_tiles_generic<M>(ctx, X, ncols, col0, logM, bc, S, spl, cp, st);
  }
  // ... and above: F_node = F_left + (x^h + d) * F_right with d * F_right as a block convolution
  for (int l = bc + 1; l <= logM; l++) {
    a.l = l;
    a.units = (int)(Mlen >> l);
    a.nxb = a.nyb = (int)(((size_t)1 << (l - 1)) / B);
    a.nk = 2 * a.nxb - 1;
    if (l == logM)
      bc_conv<BS_RIGHT, BY_D, BD_COMBINE_CANON, M>(ctx, a, ncols, (size_t)1 << l, cp, st);
    else
      bc_conv<BS_RIGHT, BY_D, BD_COMBINE, M>(ctx, a, ncols, (size_t)1 << l, cp, st);
  }
}

template <class M>
void bc_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A, const typename ArithOf<M>::T *Bc,
                 typename ArithOf<M>::T *H, size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2,
                 const uint64_t *d3, const ColMap &cm, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  using CPS = ColPlansT<M>;
  const int logM = P->logM, bc = P->bcLog;
  const size_t Mlen = P->M, B = (size_t)1 << (bc - 1), B2 = 2 * B, nb = Mlen / B;
  T *Xhat = (T *)ws_get(ctx, WS_PASS_A, ncols * 2 * Mlen * sizeof(T));
  T *Wc = (T *)ws_get(ctx, WS_PASS_B, ncols * 4 * Mlen * sizeof(T));
  T *Yhat = (T *)ws_get(ctx, WS_BC_SPECTRA, ncols * 2 * Mlen * sizeof(T));
  T *Pbuf = (T *)ws_get(ctx, WS_BC_PRODUCTS, ncols * 2 * Mlen * sizeof(T));
  BcArgs a{};
  a.bcLog = bc;
  a.logM = logM;
  a.m = (int)P->m;
  a.col0 = col0;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  a.units = 1;
  a.nxb = a.nyb = (int)nb;
  // spectra of B's blocks (the "other operand" of the data x data product): a forward pass on its own
  {
    BcArgs b = a;
    b.src = Bc;
    b.Xhat = Yhat;
    const size_t lds = padded_len(B2) * sizeof(uint64_t);
    ProfScope prof(ctx, st, "bc_fwd_kernel", (double)ncols * nb * (double)B2 * 12.0, (double)ncols * nb * ntt_fp64((double)B2, bc));
    set_max_dyn_lds((const void *)bc_fwd_kernel<BS_CENTER, CPS>, (int)lds);
    hipLaunchKernelGGL((bc_fwd_kernel<BS_CENTER, CPS>), dim3((unsigned)(ncols * nb)), dim3(col_threads(B2)), lds, st, b, cp);
  }
  // P = A * B, 2M coefficients
  a.src = A;
  a.Xhat = Xhat;
  a.Yhat = Yhat;
  a.Wc = Wc;
  a.dst = Pbuf;
  a.nk = 2 * (int)nb - 1;
  bc_conv<BS_CENTER, BY_DATA, BD_PLAIN_SCALED, M>(ctx, a, ncols, 2 * Mlen, cp, st);
  // U = rev(P) * rev(Z)^-1 mod x^(m-1);  H_j = U_{m-2-j}
  a.src = Pbuf;
  a.dst = H;
  a.nk = (int)nb;
  bc_conv<BS_REVTRUNC, BY_S, BD_HFIN, M>(ctx, a, ncols, Mlen, cp, st);
  launch_h_patch<M>(ctx, P, cp, H, A, Bc, ncols, col0, S, spl, d1, d2, d3, cm, st);
}

// one two-dimensional block convolution of `ncols * units` operands of Y/2 blocks each.  MODE 2: against the table
// `tab` ([units][Y][2B] per limb, limbs from limb0 on); MODE 3: against the data spectra `other` ([ncols*units][Y][2][B], same
// layout as Ws); MODE 0: forward only (Ws receives the spectra; no sink).
// skip_fwd / skip_inv: the transform across blocks at that end is run by a turn kernel (bc2_level_turn_kernel, bc2_h_turn_kernel)
template <int SRC, int DST, int MODE>
static void bc2_conv(rs_ctx *ctx, Bc2Args a, int logY, size_t ncols, const TabPtrs *tab, const double *other, const ColPlans &cp,
                     hipStream_t st, bool skip_fwd = false, bool skip_inv = false) {
  const size_t Y = (size_t)1 << logY, cu = ncols * (size_t)a.units;
  const dim3 grid((unsigned)(BC2_B / 2 / 256), (unsigned)cu);
  // Y <= 32: the transform across blocks in one thread's registers; Y = 64 .. 256 (M >= 2^18): in two levels
  RS_REQUIRE(cu <= 65535 && logY >= 2 && logY <= 8, "two-dimensional block convolution out of range");
  const dim3 grid_parts(grid.x << std::max(0, logY - 5), grid.y);  // one workgroup per (position range, part of 32 blocks)
  if (!skip_fwd) {
    // words: the Y/2 source blocks (read once per part in the two-level form) + Y blocks written
    const double reads = logY > 5 ? (double)(Y / 2) * (double)(1 << (logY - 5)) : (double)(Y / 2);
    ProfScope prof(ctx, st, logY > 5 ? "bc2_yfwd_big_kernel" : "bc2_yfwd_kernel", (double)cu * ((double)Y + reads) * BC2_B * 8.0,
                   (double)cu * BC2_B * ntt_fp64((double)Y, logY));
    switch (logY) {
      case 2: hipLaunchKernelGGL((bc2_yfwd_kernel<SRC, 2>), grid, dim3(256), 0, st, a, cp); break;
      case 3: hipLaunchKernelGGL((bc2_yfwd_kernel<SRC, 3>), grid, dim3(256), 0, st, a, cp); break;
      case 4: hipLaunchKernelGGL((bc2_yfwd_kernel<SRC, 4>), grid, dim3(256), 0, st, a, cp); break;
      case 5: hipLaunchKernelGGL((bc2_yfwd_kernel<SRC, 5>), grid, dim3(256), 0, st, a, cp); break;
      case 6: hipLaunchKernelGGL((bc2_yfwd_big_kernel<SRC, 1>), grid_parts, dim3(256), 0, st, a, cp); break;
      case 7: hipLaunchKernelGGL((bc2_yfwd_big_kernel<SRC, 2>), grid_parts, dim3(256), 0, st, a, cp); break;
      default: hipLaunchKernelGGL((bc2_yfwd_big_kernel<SRC, 3>), grid_parts, dim3(256), 0, st, a, cp); break;
    }
  }
  {
    const unsigned long long nb = (unsigned long long)(cu * Y * 2);
    const double Bn = (double)BC2_B;
    static const char *const names[4] = {"sub_ntt_wide_kernel<0, 0>", "sub_ntt_wide_kernel<1, 0>", "sub_ntt_wide_kernel<2, 0>", "sub_ntt_wide_kernel<3, 0>"};
    ProfScope prof(ctx, st, names[MODE], (double)nb * Bn * (MODE == 3 ? 24.0 : 16.0),
                   (double)nb * ((MODE >= 2 ? 2.0 : 1.0) * ntt_fp64(Bn, BC2_LOGB) + (MODE >= 2 ? 7.0 * Bn : 0.0)));
    TabPtrs tp{};
    if (MODE == 2) tp = *tab;
    if (MODE == 3) tp.t[0] = other;
    launch_sub_wide_bc2(MODE, a.Ws, tp, (unsigned)((size_t)a.units * Y * 2), a.col0, a.S, a.slots_per_limb, cp, nb, (const double *)a.Wy, st);
  }
  if (skip_inv) {
    RS_HIP(hipGetLastError());
    return;
  }
  if (MODE != 0 && logY <= 5) {
    ProfScope prof(ctx, st, "bc2_yinv_kernel", (double)cu * (double)Y * BC2_B * 24.0, (double)cu * 2.0 * BC2_B * ntt_fp64((double)Y, logY));
    switch (logY) {
      case 2: hipLaunchKernelGGL((bc2_yinv_kernel<DST, 2>), grid, dim3(256), 0, st, a, cp); break;
      case 3: hipLaunchKernelGGL((bc2_yinv_kernel<DST, 3>), grid, dim3(256), 0, st, a, cp); break;
      case 4: hipLaunchKernelGGL((bc2_yinv_kernel<DST, 4>), grid, dim3(256), 0, st, a, cp); break;
      default: hipLaunchKernelGGL((bc2_yinv_kernel<DST, 5>), grid, dim3(256), 0, st, a, cp); break;
    }
  } else if (MODE != 0) {
    {  // in place on Ws: 2 x Y x 2B words
      ProfScope prof(ctx, st, "bc2_yinv_a_kernel", (double)cu * (double)Y * BC2_B * 32.0, (double)cu * 2.0 * BC2_B * ntt_fp64((double)Y, 5));
      switch (logY) {
        case 6: hipLaunchKernelGGL((bc2_yinv_a_kernel<1>), grid_parts, dim3(256), 0, st, a, cp); break;
        case 7: hipLaunchKernelGGL((bc2_yinv_a_kernel<2>), grid_parts, dim3(256), 0, st, a, cp); break;
        default: hipLaunchKernelGGL((bc2_yinv_a_kernel<3>), grid_parts, dim3(256), 0, st, a, cp); break;
      }
    }
    const dim3 grid32(grid.x * 32, grid.y);
    ProfScope prof(ctx, st, "bc2_yinv_b_kernel", (double)cu * (double)Y * BC2_B * 24.0, (double)cu * 2.0 * BC2_B * ntt_fp64((double)Y, logY - 5));
    switch (logY) {
      case 6: hipLaunchKernelGGL((bc2_yinv_b_kernel<DST, 1>), grid32, dim3(256), 0, st, a, cp); break;
      case 7: hipLaunchKernelGGL((bc2_yinv_b_kernel<DST, 2>), grid32, dim3(256), 0, st, a, cp); break;
      default: hipLaunchKernelGGL((bc2_yinv_b_kernel<DST, 3>), grid32, dim3(256), 0, st, a, cp); break;
    }
  }
  RS_HIP(hipGetLastError());
}

// ---- two-dimensional block convolutions: host side ----------------------------------------------------------
// workspaces: Wy [ncols][2M] and Ws [ncols][4M] words per convolution in flight (+ the same again and a [ncols][2M]
// product buffer for H); bc_chunk_cols keeps a chunk of columns within ~6 GiB
void bc2_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, double *X, size_t ncols, size_t col0, size_t S, size_t spl,
                       int limb0, hipStream_t st, int phases) {  // phases: as big_interp
  const int logM = P->logM;
  const size_t Mlen = P->M;
  Bc2Args a{};
  a.src = X;
  a.dst = X;
  if (phases & 5) {  // the tree tiles work in place: no workspace (and `ncols` may then be a whole chunk)
    a.Wy = (double *)ws_get(ctx, WS_PASS_A, ncols * 2 * Mlen * sizeof(double));
    a.Ws = (double *)ws_get(ctx, WS_PASS_B, ncols * 4 * Mlen * sizeof(double));
  }
  a.logM = logM;
  a.m = (int)P->m;
  a.col0 = col0;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  TabPtrs tp{};
  if (phases & 1) {
    // values -> Newton coefficients: low M terms of (y_k / k!) * ((-1)^k / k!)
    a.units = 1;
    for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = P->limb[i].d_b2_e;
    bc2_conv<BS_SCALE, BD_NEWTON, 2>(ctx, a, logM + 1 - BC2_LOGB, ncols, &tp, nullptr, cp, st);
  }
  // product tree: levels <= 14 inside LDS tiles, the levels above as block convolutions F_node = F_left + (x^h + d) * F_right
  if (phases & 2)
    launch_tree_tiles(ctx, X, ncols, col0, logM, (g_tune.witness_tree_ct == 2 && g_tune.witness_tree_log >= 14) ? 14 : 13, S, spl, cp, st);
  if (!(phases & 4)) return;
  const int first = (g_tune.witness_tree_ct == 2 && g_tune.witness_tree_log >= 14) ? 15 : 14;
  bool fwd_done = false;  // this level's transform across blocks was run by the previous level's turn
  for (int l = first; l <= logM; l++) {
    a.l = l;
    a.units = (int)(Mlen >> l);
    for (int i = limb0; i < ctx->L; i++)
      tp.t[i - limb0] = static_cast<const double *>(P->limb[i].d_b2_d) + (size_t)(l - P->bcLog - 1) * 2 * Mlen;
    if (l == logM) {
      bc2_conv<BS_RIGHT, BD_COMBINE_CANON, 2>(ctx, a, l - BC2_LOGB, ncols, &tp, nullptr, cp, st, fwd_done);
      fwd_done = false;
      continue;
    }
    // level l's inverse transform across blocks + sink and level l + 1's source + forward transform as one pass
    // (bc2_level_turn_kernel; one-level transforms: the parent has at most 32 blocks)
    const int logYc = l - BC2_LOGB;
    const bool turn = g_tune.witness_level_turn && logYc >= 2 && logYc <= 4 && (size_t)ncols * (size_t)(a.units / 2) <= 65535;
    bc2_conv<BS_RIGHT, BD_COMBINE, 2>(ctx, a, logYc, ncols, &tp, nullptr, cp, st, fwd_done, turn);
    fwd_done = turn;
    if (turn) {
      const size_t cpn = ncols * (size_t)(a.units / 2), Yp = (size_t)2 << logYc;
      const dim3 grid((unsigned)(BC2_B / 2 / 256), (unsigned)cpn);
      // words per parent and position: both children's spectra read (2 Yc x 2), their lower halves... the children read, the left written, Wy written
      ProfScope prof(ctx, st, "bc2_level_turn_kernel", (double)cpn * BC2_B * 8.0 * (2.0 * Yp + 1.5 * Yp + Yp),
                     (double)cpn * BC2_B * (2.0 * ntt_fp64((double)(Yp / 2), logYc) * 2.0 + ntt_fp64((double)Yp, logYc + 1)));
      switch (logYc) {
        case 2: hipLaunchKernelGGL((bc2_level_turn_kernel<2>), grid, dim3(256), 0, st, a, cp); break;
        case 3: hipLaunchKernelGGL((bc2_level_turn_kernel<3>), grid, dim3(256), 0, st, a, cp); break;
        default: hipLaunchKernelGGL((bc2_level_turn_kernel<4>), grid, dim3(256), 0, st, a, cp); break;
      }
      RS_HIP(hipGetLastError());
    }
  }
}

void bc2_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, const double *A, const double *Bc, double *H, size_t ncols,
                  size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, int limb0,
                  hipStream_t st) {
  const int logM = P->logM, logY = logM + 1 - BC2_LOGB;
  const size_t Mlen = P->M;
  double *Wy = (double *)ws_get(ctx, WS_PASS_A, ncols * 2 * Mlen * sizeof(double));
  double *Ws = (double *)ws_get(ctx, WS_PASS_B, ncols * 4 * Mlen * sizeof(double));
  double *WsA = (double *)ws_get(ctx, WS_BC_SPECTRA, ncols * 4 * Mlen * sizeof(double));
  double *Pbuf = (double *)ws_get(ctx, WS_BC_PRODUCTS, ncols * 2 * Mlen * sizeof(double));
  Bc2Args a{};
  a.logM = logM;
  a.m = (int)P->m;
  a.col0 = col0;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  a.units = 1;
  a.Wy = Wy;
  // the two-dimensional spectrum of A ...
  a.src = A;
  a.Ws = WsA;
  bc2_conv<BS_CENTER, BD_PLAIN_SCALED, 0>(ctx, a, logY, ncols, nullptr, nullptr, cp, st);
  // ... P = A * B, 2M coefficients
  a.src = Bc;
  a.Ws = Ws;
  a.dst = Pbuf;
  // the turn of H (bc2_h_turn_kernel): the product's inverse transform across blocks and the forward one of its reversal as
  // one pass, the 2M-word product buffer neither written nor read (one-level transforms of at most 16 blocks: M <= 2^16)
  // (the turn kernel reverses around 2m - 2: needs B <= 2m - 2 < 2M, true for M = next_pow2(m) -- checked, as in launch_cross_turn)
  const bool turn = g_tune.witness_h_turn && logY >= 2 && logY <= 4 && 2 * (long long)P->m - 2 >= (long long)BC2_B &&
                    2 * (long long)P->m - 2 < ((long long)2 << logM);
  bc2_conv<BS_CENTER, BD_PLAIN_SCALED, 3>(ctx, a, logY, ncols, nullptr, WsA, cp, st, false, turn);
  if (turn) {
    const size_t Y = (size_t)1 << logY;
    const dim3 grid((unsigned)(BC2_B / 2 / 256), (unsigned)ncols);
    ProfScope prof(ctx, st, "bc2_h_turn_kernel", (double)ncols * BC2_B * 8.0 * (2.0 * Y + Y), (double)ncols * BC2_B * 3.0 * ntt_fp64((double)Y, logY));
    switch (logY) {
      case 2: hipLaunchKernelGGL((bc2_h_turn_kernel<2>), grid, dim3(256), 0, st, a, cp); break;
      case 3: hipLaunchKernelGGL((bc2_h_turn_kernel<3>), grid, dim3(256), 0, st, a, cp); break;
      default: hipLaunchKernelGGL((bc2_h_turn_kernel<4>), grid, dim3(256), 0, st, a, cp); break;
    }
    RS_HIP(hipGetLastError());
  }
  // U = rev(P) * rev(Z)^-1 mod x^(m-1);  H_j = U_{m-2-j}
  TabPtrs tp{};
  for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = P->limb[i].d_b2_s;
  a.src = Pbuf;
  a.dst = H;
  bc2_conv<BS_REVTRUNC, BD_HFIN, 2>(ctx, a, logY, ncols, &tp, nullptr, cp, st, turn);
  launch_h_patch<Mod>(ctx, P, cp, H, A, Bc, ncols, col0, S, spl, d1, d2, d3, cm, st);
}

#define RS_INSTANTIATE(M)                                                                                                                     \
  template void bc_interp<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, ArithOf<M>::T *, size_t, size_t, size_t, size_t, hipStream_t); \
  template void bc_h<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, const ArithOf<M>::T *, const ArithOf<M>::T *, ArithOf<M>::T *,    \
                        size_t, size_t, size_t, size_t, const uint64_t *, const uint64_t *, const uint64_t *, const ColMap &, hipStream_t);
RS_INSTANTIATE(Mod)
RS_INSTANTIATE(ModI)
#undef RS_INSTANTIATE

// The generic sub-transform kernel of the multi-pass path (witness_big.hip, launch_sub_inc): `mode` is sub_ntt_kernel's MODE
// (0, 2, 3 or 4); it reads every column's inc from its plan.  The caller holds the ProfScope.
template <class M>
void launch_sub_generic(int mode, typename ArithOf<M>::T *X, size_t nblocks, int logB, int log_n1, const TabPtrs &tp, size_t tab_period,
                        size_t bpc, size_t col0, size_t S, size_t spl, const ColPlansT<M> &cp, size_t lds, hipStream_t st) {
  const int thr = (int)std::max<size_t>(64, std::min<size_t>(1024, ((size_t)1 << logB) / 16));
#define RS_SUB_LAUNCH(MODE)                                                                                                     \
  do {                                                                                                                          \
    set_max_dyn_lds((const void *)sub_ntt_kernel<MODE, ColPlansT<M>>, (int)lds);                                                \
    hipLaunchKernelGGL((sub_ntt_kernel<MODE, ColPlansT<M>>), dim3((unsigned)nblocks), dim3(thr), lds, st, X, logB, log_n1, tp,  \
                       (unsigned)std::max<size_t>(1, tab_period), (unsigned)bpc, col0, (unsigned)S, (unsigned)spl, cp);         \
  } while (0)
  switch (mode) {
    case 0: RS_SUB_LAUNCH(0); break;
    case 2: RS_SUB_LAUNCH(2); break;
    case 3: RS_SUB_LAUNCH(3); break;
    case 4: RS_SUB_LAUNCH(4); break;
    default: RS_REQUIRE(false, "internal: generic sub-transform launch: mode must be 0, 2, 3 or 4");
  }
#undef RS_SUB_LAUNCH
  RS_HIP(hipGetLastError());
}
template void launch_sub_generic<Mod>(int, double *, size_t, int, int, const TabPtrs &, size_t, size_t, size_t, size_t, size_t, const ColPlans &, size_t, hipStream_t);
template void launch_sub_generic<ModI>(int, uint64_t *, size_t, int, int, const TabPtrs &, size_t, size_t, size_t, size_t, size_t, const ColPlansT<ModI> &,
                                       size_t, hipStream_t);

}  // namespace rs
