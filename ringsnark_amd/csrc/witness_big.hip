// witness_big.hip -- the multi-pass path of the witness map (M > 2^14, or an incomplete plan): cross passes over global memory
// and rooted sub-transforms, the levels of the product tree above its tiles, and the two forms of H (witness.hip has the map
// of the units).  The launch helpers templated on <INV, MODE, ...> stay inside this unit.
#include <algorithm>
#include <string>
#include <type_traits>

#include "witness_launch.hpp"
#include "witness_multipass.hpp"

namespace rs {

template <bool INV, int MODE, class M, int V>
static void launch_cross_pass(int R, const dim3 &grid, const CrossArgs &a, const ColPlansT<M> &cp, hipStream_t st) {
  using CPS = ColPlansT<M>;
  if constexpr (std::is_same<M, Mod>::value) {  // radix 32 / 64 passes: six cross stages (M = 2^18) in ONE pass over the workspace instead of two
    if (R == 6) {
      hipLaunchKernelGGL((cross_kernel<INV, 6, MODE, CPS, 1>), grid, dim3(256), 0, st, a, cp);  // 64 elements per thread already
      return;
    }
    if (R == 5) {
      hipLaunchKernelGGL((cross_kernel<INV, 5, MODE, CPS, V>), grid, dim3(256), 0, st, a, cp);
      return;
    }
  }
  switch (R) {
    case 4: hipLaunchKernelGGL((cross_kernel<INV, 4, MODE, CPS, V>), grid, dim3(256), 0, st, a, cp); break;
    case 3: hipLaunchKernelGGL((cross_kernel<INV, 3, MODE, CPS, V>), grid, dim3(256), 0, st, a, cp); break;
    case 2: hipLaunchKernelGGL((cross_kernel<INV, 2, MODE, CPS, V>), grid, dim3(256), 0, st, a, cp); break;
    default: hipLaunchKernelGGL((cross_kernel<INV, 1, MODE, CPS, V>), grid, dim3(256), 0, st, a, cp); break;
  }
}

// Cross stages of the length-2^logsub transforms in W[ncols][2^logtot]: forward stages
// [0, logsub-logB) (the first pass reads through source MODE from a.src), or inverse stages
// [logB, logsub) (the last pass writes through sink MODE to a.dst).
// algorithmic 8-byte words per column of a cross pass that reads through source / writes through sink MODE
template <bool INV, int MODE>
static double cross_words(const CrossArgs &a, bool special) {
  const double n = (double)((size_t)1 << a.logtot), M = (double)((size_t)1 << a.logM);
  if (!special || MODE == 0) return 2.0 * n;
  if (!INV) return n + (MODE == CS_FILL_RIGHT ? M / 2.0 : M);                  // source words + workspace written
  return n + (MODE == CD_COMBINE || MODE == CD_COMBINE_CANON ? 1.5 * M : M);  // workspace read + sink traffic
}
// profile name of one instantiation, as rocprofv3 prints it ("rs::cross_kernel<false, 4, 1, ..."): static storage
static const char *cross_name(bool inv, int R, int mode) {
  static std::mutex mu;
  static std::map<int, std::string> names;
  std::lock_guard<std::mutex> lk(mu);
  const int key = (inv ? 1 : 0) | (R << 1) | (mode << 8);
  auto it = names.find(key);
  if (it == names.end())
    it = names.emplace(key, std::string("cross_kernel<") + (inv ? "true" : "false") + ", " + std::to_string(R) + ", " + std::to_string(mode) + ",").first;
  return it->second.c_str();
}
template <bool INV, int MODE, class M>
static void launch_cross(rs_ctx *ctx, CrossArgs a, size_t ncols, int logB, const ColPlansT<M> &cp, hipStream_t st) {
  const int ncross = a.logsub - logB;
  const size_t groups = ((size_t)1 << a.logtot);
  int done = 0;
  while (done < ncross) {
    // FP64: up to six stages per pass (64 strided elements per thread: the pass is HBM bound, the registers are idle) --
    // a transform with five or six cross stages (M = 2^17, 2^18) crosses the workspace once instead of twice
    const int R = pick_radix(ncross - done, std::is_same<M, Mod>::value ? std::max(1, std::min(6, g_tune.witness_cross_maxr)) : 4);
    a.s0 = INV ? logB + done : done;
    const bool special = INV ? (done + R >= ncross) : (done == 0);
    // two adjacent groups per thread, 16-byte accesses (cross_kernel<..., 2>): needs wave-uniform twiddles for 128
    // consecutive groups (smallest gap >= 2^7) and 16-byte aligned columns
    const bool paired = g_tune.witness_cross_pair && R <= 5 && logB >= 8 && a.logM >= 2 &&
                        (((uintptr_t)a.W | (uintptr_t)a.src | (uintptr_t)a.dst) & 15) == 0;
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((groups >> R) / (paired ? 512 : 256), 1024));
    const dim3 grid(gx, (unsigned)ncols);
    ProfScope prof(ctx, st, cross_name(INV, R, special ? MODE : 0), (double)ncols * 8.0 * cross_words<INV, MODE>(a, special),
                   (double)ncols * ntt_fp64((double)groups, (special && !INV) ? R - 1 : R));  // a source pass: stage 0 meets zero padding, a copy
    if (special && paired)
      launch_cross_pass<INV, MODE, M, 2>(R, grid, a, cp, st);
    else if (special)
      launch_cross_pass<INV, MODE, M, 1>(R, grid, a, cp, st);
    else if (paired)
      launch_cross_pass<INV, 0, M, 2>(R, grid, a, cp, st);
    else
      launch_cross_pass<INV, 0, M, 1>(R, grid, a, cp, st);
    done += R;
  }
  RS_HIP(hipGetLastError());
}

// Block of the rooted sub-transforms of a multi-pass transform of length 2^logsub: the LDS tile (2^13), or 2^12 for the
// FP64 contexts (knob witness_sub_log = 12; sub_ntt_w12_kernel, four workgroups per CU: 14 % faster per coefficient)
// where the extra cross stage keeps the cross pass at four stages or fewer (knob witness_sub12_cross) -- a five-stage
// FORWARD pass from a source costs more than the smaller block saves (measured on the headline).
template <class M>
static int sub_block_log(int logT, int logsub) {
  return (std::is_same<M, Mod>::value && g_tune.witness_sub_log == 12 && logT == 13 && logsub - 12 <= g_tune.witness_sub12_cross) ? 12 : logT;
}

// FP64 instructions per coefficient of the pointwise step of a fused sub-transform: one modular product, or (incomplete
// transforms, witness_inc.hpp) 2^inc of them, their sums and reductions, and the product with eta
static double pointwise_fp64(int inc) { return inc ? 7.0 * (double)(1 << inc) + 13.0 : 7.0; }

// `inc`: stages every transform of this launch stops short (the same for every column: launch_sub splits otherwise)
template <int MODE, class M>
static void launch_sub_inc(rs_ctx *ctx, typename ArithOf<M>::T *X, size_t ncols, size_t col0, int logtot, int logsub, int logB,
                           const TabPtrs *tabs, size_t tab_period, size_t S, size_t spl, const ColPlansT<M> &cp, hipStream_t st, int inc) {
  constexpr bool FP = std::is_same<M, Mod>::value;
  const size_t lds = padded_len((size_t)1 << logB) * sizeof(double);
  const size_t bpc = (size_t)1 << (logtot - logB);
  static const char *const names[5] = {"sub_ntt_kernel<0", "sub_ntt_kernel<1", "sub_ntt_kernel<2", "sub_ntt_kernel<3", "sub_ntt_kernel<4"};
  // names as rocprofv3 prints them: "sub_ntt_wide_kernel<MODE, INC>"
  static const char *const names_wide[5][5] = {
      {"sub_ntt_wide_kernel<0, 0>", "sub_ntt_wide_kernel<0, 1>", "sub_ntt_wide_kernel<0, 2>", "sub_ntt_wide_kernel<0, 3>", "sub_ntt_wide_kernel<0, 4>"},
      {"sub_ntt_wide_kernel<1, 0>", "", "", "", ""},
      {"sub_ntt_wide_kernel<2, 0>", "sub_ntt_wide_kernel<2, 1>", "sub_ntt_wide_kernel<2, 2>", "sub_ntt_wide_kernel<2, 3>", "sub_ntt_wide_kernel<2, 4>"},
      {"sub_ntt_wide_kernel<3, 0>", "sub_ntt_wide_kernel<3, 1>", "sub_ntt_wide_kernel<3, 2>", "sub_ntt_wide_kernel<3, 3>", "sub_ntt_wide_kernel<3, 4>"},
      {"sub_ntt_wide_kernel<4, 0>", "", "", "", ""}};
  static const char *const names_w12[5][5] = {
      {"sub_ntt_w12_kernel<0, 0>", "sub_ntt_w12_kernel<0, 1>", "sub_ntt_w12_kernel<0, 2>", "sub_ntt_w12_kernel<0, 3>", "sub_ntt_w12_kernel<0, 4>"},
      {"sub_ntt_w12_kernel<1, 0>", "", "", "", ""},
      {"sub_ntt_w12_kernel<2, 0>", "sub_ntt_w12_kernel<2, 1>", "sub_ntt_w12_kernel<2, 2>", "sub_ntt_w12_kernel<2, 3>", "sub_ntt_w12_kernel<2, 4>"},
      {"sub_ntt_w12_kernel<3, 0>", "sub_ntt_w12_kernel<3, 1>", "sub_ntt_w12_kernel<3, 2>", "sub_ntt_w12_kernel<3, 3>", "sub_ntt_w12_kernel<3, 4>"},
      {"sub_ntt_w12_kernel<4, 0>", "", "", "", ""}};
  RS_REQUIRE(inc >= 0 && inc <= RS_INC_MAX && (inc == 0 || (MODE != 1 && MODE != 4)) && logB > inc, "internal: sub-transform launch out of range");
  const bool ct = FP && logB == 13 && MODE != 1 && g_tune.witness_sub_ct == 2;  // 0: the generic kernel
  const double Bn = (double)((size_t)1 << logB), blocks = (double)(ncols * bpc);
  const bool w12 = FP && logB == 12 && MODE != 1 && g_tune.witness_sub_log == 12;
  ProfScope prof(ctx, st, w12 ? names_w12[MODE][inc] : ct ? names_wide[MODE][inc] : names[MODE], blocks * Bn * (MODE == 4 ? 32.0 : MODE == 3 ? 24.0 : 16.0),
                 blocks * ((MODE >= 2 ? 2.0 : 1.0) * ntt_fp64(Bn, logB - inc) + (MODE == 4 ? 24.0 * Bn : MODE >= 2 ? pointwise_fp64(inc) * Bn : 0.0)));
  static TabPtrs none{};
  const TabPtrs &tp = tabs ? *tabs : none;
  if constexpr (FP) {
    const unsigned long long nb = (unsigned long long)(ncols * bpc);
    if (logB == 12 && MODE != 1 && g_tune.witness_sub_log == 12) {
      const int wl = 4352 * (int)sizeof(double);
#define RS_W12_LAUNCH(INC)                                                                                                              \
  hipLaunchKernelGGL((sub_ntt_w12_kernel<MODE, INC>), dim3((unsigned)std::min<unsigned long long>(nb, 1024)), dim3(256), wl, st, X,     \
                     logsub - logB, tp, (unsigned)std::max<size_t>(1, tab_period), (unsigned)bpc, col0, (unsigned)S, (unsigned)spl, cp, nb)
      if constexpr (MODE == 4) {
        RS_W12_LAUNCH(0);
      } else {
        switch (inc) {
          case 0: RS_W12_LAUNCH(0); break;
          case 1: RS_W12_LAUNCH(1); break;
          case 2: RS_W12_LAUNCH(2); break;
          case 3: RS_W12_LAUNCH(3); break;
          default: RS_W12_LAUNCH(4); break;
        }
      }
#undef RS_W12_LAUNCH
      RS_HIP(hipGetLastError());
      return;
    }
    if (logB == 13 && MODE != 1 && g_tune.witness_sub_ct == 2) {
      const int wl = (int)(WideShape<13>::TILE * sizeof(double));
#define RS_WIDE_LAUNCH(INC)                                                                                                             \
  do {                                                                                                                                  \
    set_max_dyn_lds((const void *)sub_ntt_wide_kernel<MODE, INC>, wl);                                                                  \
    hipLaunchKernelGGL((sub_ntt_wide_kernel<MODE, INC>), dim3((unsigned)std::min<unsigned long long>(nb, 512)), dim3(256), wl, st, X,   \
                       logsub - logB, tp, (unsigned)std::max<size_t>(1, tab_period), (unsigned)bpc, col0, (unsigned)S, (unsigned)spl, cp, \
                       nb, (const double *)nullptr);                                                                                    \
  } while (0)
      if constexpr (MODE == 4) {
        RS_WIDE_LAUNCH(0);
      } else {
        switch (inc) {
          case 0: RS_WIDE_LAUNCH(0); break;
          case 1: RS_WIDE_LAUNCH(1); break;
          case 2: RS_WIDE_LAUNCH(2); break;
          case 3: RS_WIDE_LAUNCH(3); break;
          default: RS_WIDE_LAUNCH(4); break;
        }
      }
#undef RS_WIDE_LAUNCH
      RS_HIP(hipGetLastError());
      return;
    }
  }
  // the generic kernel reads every column's inc from its plan
  launch_sub_generic<M>(MODE, X, ncols * bpc, logB, logsub - logB, tp, tab_period, bpc, col0, S, spl, cp, lds, st);
}

// Sub-transforms of the length-2^logsub transforms in X[ncols][2^logtot].  The tuned kernels take the number of stages an
// incomplete transform stops short as a template parameter, so columns of primes with different 2-adicity (column c belongs
// to limb ((col0 + c) % S) / spl) go in separate launches -- one launch whenever they agree (always at the headline, where a
// chunk of columns is one limb).
template <int MODE, class M>
static void launch_sub(rs_ctx *ctx, typename ArithOf<M>::T *X, size_t ncols, size_t col0, int logtot, int logsub, int logB,
                       const TabPtrs *tabs, size_t tab_period, size_t S, size_t spl, const ColPlansT<M> &cp, hipStream_t st) {
  auto inc_at = [&](size_t c) { return cp.l[((col0 + c) % S) / spl].inc(logsub); };
  bool same = true;
  for (size_t c = 0; c < ncols && same; c += spl - (col0 + c) % spl) same = inc_at(c) == inc_at(0);
  if (same) {
    launch_sub_inc<MODE, M>(ctx, X, ncols, col0, logtot, logsub, logB, tabs, tab_period, S, spl, cp, st, ncols ? inc_at(0) : 0);
    return;
  }
  for (size_t c = 0; c < ncols;) {
    size_t e = std::min(ncols, c + spl - (col0 + c) % spl);
    while (e < ncols && inc_at(e) == inc_at(c)) e = std::min(ncols, e + spl);  // neighbouring limbs that agree: one launch
    TabPtrs tp = tabs ? *tabs : TabPtrs{};
    if (MODE == 3 && tabs) tp.t[0] = static_cast<const typename ArithOf<M>::T *>(tabs->t[0]) + (c << logtot);  // the other workspace: same shape as X
    launch_sub_inc<MODE, M>(ctx, X + (c << logtot), e - c, col0 + c, logtot, logsub, logB, tabs ? &tp : nullptr, tab_period, S, spl, cp, st, inc_at(c));
    c = e;
  }
}

// The 2^13 sub-transforms of a two-dimensional block convolution (witness_lds.hip, bc2_conv): `nb` blocks of Ws, block b reading
// block b >> 1 of Wy; `mode` is sub_ntt_wide_kernel's MODE (0, 2 or 3).  The caller holds the ProfScope.
void launch_sub_wide_bc2(int mode, double *Ws, const TabPtrs &tp, unsigned period, size_t col0, unsigned S, unsigned spl, const ColPlans &cp,
                         unsigned long long nb, const double *Wy, hipStream_t st) {
  const int wl = (int)(WideShape<13>::TILE * sizeof(double));
#define RS_WIDE_LAUNCH(MODE)                                                                                                            \
  do {                                                                                                                                  \
    set_max_dyn_lds((const void *)sub_ntt_wide_kernel<MODE>, wl);                                                                       \
    hipLaunchKernelGGL((sub_ntt_wide_kernel<MODE>), dim3((unsigned)std::min<unsigned long long>(nb, 512)), dim3(256), wl, st, Ws, 1, tp, \
                       period, period, col0, S, spl, cp, nb, Wy);                                                                       \
  } while (0)
  switch (mode) {
    case 0: RS_WIDE_LAUNCH(0); break;
    case 2: RS_WIDE_LAUNCH(2); break;
    case 3: RS_WIDE_LAUNCH(3); break;
    default: RS_REQUIRE(false, "internal: sub-transform launch of a block convolution: mode must be 0, 2 or 3");
  }
#undef RS_WIDE_LAUNCH
}

// The turn of H as one pass (cross_turn_kernel): reads a.W (the product's workspace, sub-transformed), writes a.dst (the
// workspace of T = rev(P) mod x^(m-1), cross stages done).  Returns false when the two transforms need more than one cross
// pass each (the caller then runs the two passes).
template <class M>
static bool launch_cross_turn(rs_ctx *ctx, CrossArgs a, size_t ncols, int logB, const ColPlansT<M> &cp, hipStream_t st) {
  using CPS = ColPlansT<M>;
  constexpr bool FP = std::is_same<M, Mod>::value;
  const int R = a.logtot - logB;
  const int maxr = FP ? std::max(1, std::min(6, g_tune.witness_cross_maxr)) : 4;
  if (!g_tune.witness_h_turn || R < 1 || R > maxr || a.logsub != a.logtot || logB < 8) return false;
  if ((((uintptr_t)a.W | (uintptr_t)a.dst) & 15) != 0) return false;
  // cross_turn_kernel indexes the product at i0 = 2m - 2 - j - c >= 0 and shifts by E - 1 - (i0 >> logB) >= 0: holds for
  // M = next_pow2(m) (2m - 2 >= M >= B, 2m - 2 < 2M = 2^logtot) -- enforced, not assumed (round-5 advice): else the two passes
  if (2 * (long long)a.m - 2 < ((long long)1 << logB) || 2 * (long long)a.m - 2 >= ((long long)1 << a.logtot)) return false;
  const size_t B = (size_t)1 << logB;
  const bool pair = R <= 5;
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((B / (pair ? 2 : 1)) / 256, 1024));
  const dim3 grid(gx, (unsigned)ncols);
  const double n = (double)((size_t)1 << a.logtot);
  static const char *const names[7] = {"", "cross_turn_kernel<1", "cross_turn_kernel<2", "cross_turn_kernel<3", "cross_turn_kernel<4", "cross_turn_kernel<5",
                                       "cross_turn_kernel<6"};
  ProfScope prof(ctx, st, names[R], (double)ncols * 8.0 * 2.0 * n, (double)ncols * (ntt_fp64(n, R) + ntt_fp64(n, R - 1)));
  switch (R) {
    case 1: hipLaunchKernelGGL((cross_turn_kernel<1, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 2: hipLaunchKernelGGL((cross_turn_kernel<2, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 3: hipLaunchKernelGGL((cross_turn_kernel<3, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 4: hipLaunchKernelGGL((cross_turn_kernel<4, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 5:
      if constexpr (FP) hipLaunchKernelGGL((cross_turn_kernel<5, CPS, 2>), grid, dim3(256), 0, st, a, cp);
      break;
    default:
      if constexpr (FP) hipLaunchKernelGGL((cross_turn_kernel<6, CPS, 1>), grid, dim3(256), 0, st, a, cp);
      break;
  }
  RS_HIP(hipGetLastError());
  return true;
}

// The turn between tree levels l = a.l and l + 1 as one pass (cross_level_turn_kernel) on the workspace a.W and the columns
// a.dst; false when the two levels differ in block size or need more than one cross pass each.
template <class M>
static bool launch_level_turn(rs_ctx *ctx, CrossArgs a, size_t ncols, int logB, int logB_next, const ColPlansT<M> &cp, hipStream_t st) {
  using CPS = ColPlansT<M>;
  constexpr bool FP = std::is_same<M, Mod>::value;
  const int RL = a.l - logB;
  const int maxr = FP ? std::max(1, std::min(6, g_tune.witness_cross_maxr)) : 4;
  if (!g_tune.witness_level_turn || logB != logB_next || RL < 1 || RL + 1 > maxr || logB < 8 || a.l + 1 > a.logtot) return false;
  if ((((uintptr_t)a.W | (uintptr_t)a.dst) & 15) != 0) return false;
  const bool pair = RL <= 3;
  const size_t groups = (((size_t)1 << a.logtot) >> (a.l + 1)) * (((size_t)1 << logB) / (pair ? 2 : 1));
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(groups / 256, 1024));
  const dim3 grid(gx, (unsigned)ncols);
  const double n = (double)((size_t)1 << a.logtot);
  static const char *const names[6] = {"", "cross_level_turn_kernel<1", "cross_level_turn_kernel<2", "cross_level_turn_kernel<3", "cross_level_turn_kernel<4",
                                       "cross_level_turn_kernel<5"};
  // words per coefficient position of the column: workspace read + written, the children's lower halves read, the left child written
  ProfScope prof(ctx, st, names[RL], (double)ncols * 8.0 * 3.0 * n, (double)ncols * (ntt_fp64(n, RL) + ntt_fp64(n / 2.0, RL)));
  switch (RL) {
    case 1: hipLaunchKernelGGL((cross_level_turn_kernel<1, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 2: hipLaunchKernelGGL((cross_level_turn_kernel<2, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 3: hipLaunchKernelGGL((cross_level_turn_kernel<3, CPS, 2>), grid, dim3(256), 0, st, a, cp); break;
    case 4:
      if constexpr (FP) hipLaunchKernelGGL((cross_level_turn_kernel<4, CPS, 1>), grid, dim3(256), 0, st, a, cp);
      break;
    default:
      if constexpr (FP) hipLaunchKernelGGL((cross_level_turn_kernel<5, CPS, 1>), grid, dim3(256), 0, st, a, cp);
      break;
  }
  RS_HIP(hipGetLastError());
  return true;
}

// g_tune.witness_tree_fwd: the tile kernel runs the forward cross stages of the first level above the tiles.  OFF by
// default -- measured (profiles/r05_knob_ab_tree_once.txt): it removes a 9.8 ms pass and costs the tile kernel 16 ms (176 ->
// 192 ms per headline proof): one workgroup per CU has nothing to hide its epilogue's LDS reads and stores behind.
// Can the wide 2^14 tile kernel run the forward cross stages of level 15 (2 or 3 of them: blocks of 2^13 / 2^12)?
template <class M>
bool tree_fwd_stages(const WitnessPlan *P) {
  if constexpr (!std::is_same<M, Mod>::value) return false;
  const int logM = P->logM, logT = std::min(g_tune.witness_lds_logM, logM);
  if (!g_tune.witness_tree_fwd || !(logT == 13 && logM >= 15 && g_tune.witness_tree_ct == 2 && g_tune.witness_tree_log >= 14)) return false;
  const int rf = 15 - sub_block_log<M>(logT, 15);
  return rf == 2 || rf == 3;
}

// multi-pass interpolation of `ncols` columns X[ncols][M] in place; W: workspace [ncols][2M].
// phases: 1 = values -> Newton coefficients, 2 = the product tree's tiles (in place on X: no workspace, so the caller may run
// it ONCE over all the columns of a chunk instead of per workspace-sized sub-chunk), 4 = the levels above the tiles.
template <class M>
// tree_fwd (phases 2 and 4 must agree): the tile kernel of the right children also runs the forward cross stages of the first
// level above the tiles, into W as [ncols][M] (tree_fwd_stages() says whether it can) -- that level's source pass is skipped.
void big_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *X, typename ArithOf<M>::T *W,
                       size_t ncols, size_t col0, size_t S, size_t spl, int limb0, hipStream_t st, int phases, bool tree_fwd) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  const int logM = P->logM, logT = std::min(g_tune.witness_lds_logM, logM);
  int logB = sub_block_log<M>(logT, logM + 1);  // block of the rooted sub-transforms
  const size_t Mlen = P->M;
  CrossArgs a{};
  a.W = W;
  a.src = X;
  a.dst = X;
  a.logM = logM;
  a.l = 1;
  a.m = (int)P->m;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  a.col0 = col0;
  TabPtrs tp{};
  if (phases & 1) {
    // values -> Newton coefficients: one cyclic convolution of length 2M
    a.logtot = a.logsub = logM + 1;
    launch_cross<false, CS_SCALE_PAD, M>(ctx, a, ncols, logB, cp, st);
    for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = P->limb[i].d_ehat;
    launch_sub<2, M>(ctx, W, ncols, col0, logM + 1, logM + 1, logB, &tp, (2 * Mlen) >> logB, S, spl, cp, st);
    launch_cross<true, CD_TAKE_LOW, M>(ctx, a, ncols, logB, cp, st);
  }
  // product tree: levels <= logTree inside LDS tiles (the wide kernel takes 2^14 tiles: one multi-pass level less)
  int logTree = logT;
  if constexpr (FP) {
    if (logT == 13 && logM >= 15 && g_tune.witness_tree_ct == 2 && g_tune.witness_tree_log >= 14) logTree = 14;
    const int rf = tree_fwd ? logTree + 1 - sub_block_log<M>(logT, logTree + 1) : 0;
    if (phases & 2) launch_tree_tiles(ctx, X, ncols, col0, logM, logTree, S, spl, cp, st, false, tree_fwd ? W : nullptr, rf);
  } else {
    if (phases & 2) launch_tree_tiles_generic<M>(ctx, X, ncols, col0, logM, logT, S, spl, cp, st);
  }
  if (!(phases & 4)) return;
  // levels above: F_node = F_left + D_left * F_right with multi-pass transforms of length 2^l
  a.logtot = logM;
  bool fwd_done = tree_fwd;  // the forward cross pass of this level was run by the previous level's turn (or by the tile kernel)
  for (int l = logTree + 1; l <= logM; l++) {
    a.l = l;
    a.logsub = l;
    logB = sub_block_log<M>(logT, l);
    if (!fwd_done) launch_cross<false, CS_FILL_RIGHT, M>(ctx, a, ncols, logB, cp, st);
    fwd_done = false;
    for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = static_cast<const T *>(P->limb[i].d_dhat) + (size_t)l * Mlen;
    launch_sub<2, M>(ctx, W, ncols, col0, logM, l, logB, &tp, Mlen >> logB, S, spl, cp, st);
    if (l == logM) {
      launch_cross<true, CD_COMBINE_CANON, M>(ctx, a, ncols, logB, cp, st);
    } else {
      // this level's last inverse cross pass and the next level's first forward pass as one pass over memory, when the
      // two levels share their block size (cross_level_turn_kernel); else the inverse pass alone
      fwd_done = launch_level_turn<M>(ctx, a, ncols, logB, sub_block_log<M>(logT, l + 1), cp, st);
      if (!fwd_done) launch_cross<true, CD_COMBINE, M>(ctx, a, ncols, logB, cp, st);
    }
  }
}

// multi-pass H = quo(A*B, Z) (+ ZK patch) for `ncols` columns; W1, W2: workspaces [ncols][2M]
template <class M>
void big_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A,
                  const typename ArithOf<M>::T *B, typename ArithOf<M>::T *H, typename ArithOf<M>::T *W1, typename ArithOf<M>::T *W2,
                  size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2, const uint64_t *d3,
                  const ColMap &cm, int limb0, hipStream_t st) {
  const int logM = P->logM, logB = sub_block_log<M>(std::min(g_tune.witness_lds_logM, logM), logM + 1);
  const size_t Mlen = P->M;
  CrossArgs a{};
  a.logM = logM;
  a.l = 1;
  a.m = (int)P->m;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  a.col0 = col0;
  a.logtot = a.logsub = logM + 1;
  TabPtrs tp{};
  // W1 = spectrum of A; W2 = A * B (spectrum product inside the sub-transform kernel of B)
  a.W = W1;
  a.src = A;
  launch_cross<false, CS_PAD_CENTER, M>(ctx, a, ncols, logB, cp, st);
  launch_sub<0, M>(ctx, W1, ncols, col0, logM + 1, logM + 1, logB, nullptr, 1, S, spl, cp, st);
  a.W = W2;
  a.src = B;
  launch_cross<false, CS_PAD_CENTER, M>(ctx, a, ncols, logB, cp, st);
  tp.t[0] = W1;
  launch_sub<3, M>(ctx, W2, ncols, col0, logM + 1, logM + 1, logB, &tp, 1, S, spl, cp, st);
  // U = rev(P) * rev(Z)^-1 mod x^(m-1): the product's last inverse cross pass and the first forward pass of its reversal are
  // one pass over memory when each transform has a single cross pass (cross_turn_kernel); otherwise the two passes
  a.dst = W1;
  const bool turned = launch_cross_turn<M>(ctx, a, ncols, logB, cp, st);  // a.W = W2 -> W1
  if (!turned) launch_cross<true, CD_PLAIN, M>(ctx, a, ncols, logB, cp, st);
  a.W = W1;
  a.src = W2;
  if (!turned) launch_cross<false, CS_REV_TRUNC, M>(ctx, a, ncols, logB, cp, st);
  for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = P->limb[i].d_shat;
  launch_sub<2, M>(ctx, W1, ncols, col0, logM + 1, logM + 1, logB, &tp, (2 * Mlen) >> logB, S, spl, cp, st);
  a.dst = H;
  if (!d1) {  // d1 = d2 = d3 = 0 (groth16.tcc:82-84): nothing to patch, the last pass writes the finished column
    launch_cross<true, CD_H_FINISH_CANON, M>(ctx, a, ncols, logB, cp, st);
    return;
  }
  launch_cross<true, CD_H_FINISH, M>(ctx, a, ncols, logB, cp, st);
  launch_h_patch<M>(ctx, P, cp, H, A, B, ncols, col0, S, spl, d1, d2, d3, cm, st);
}

// H on a coset, when C's coefficients are at hand (Rinocchio keeps C_mid, rinocchio.tcc:75-190; ringGroth16 never
// interpolates C and takes big_h): with the M points g w^i, none a root of Z,
//     H(g w^i) = (A(g w^i) B(g w^i) - C(g w^i)) / Z(g w^i),   deg H <= m - 2 < M,
// so H is the inverse coset transform of that quotient: FOUR transforms of length M (three forward, one inverse, the
// pointwise step inside the sub-transform kernel of B) instead of big_h's five of length 2M.  The division is exact in
// Z_q, so H is the polynomial the reference's long division (util/polynomials.tcc:62-81) returns; the ZK patch follows as
// in big_h.  W1, W2: workspaces [ncols][2M] (W1 holds the spectra of A and of C, W2 that of B and the result).
template <class M>
void big_h_coset(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A,
                        const typename ArithOf<M>::T *B, const typename ArithOf<M>::T *Cc, typename ArithOf<M>::T *H,
                        typename ArithOf<M>::T *W1, typename ArithOf<M>::T *W2, size_t ncols, size_t col0, size_t S, size_t spl,
                        const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, int limb0, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const int logM = P->logM, logB = sub_block_log<M>(std::min(g_tune.witness_lds_logM, logM), logM);
  const size_t Mlen = P->M;
  T *W3 = W1 + ncols * Mlen;  // the second half of the [ncols][2M] workspace
  CrossArgs a{};
  a.logM = logM;
  a.l = 1;
  a.m = (int)P->m;
  a.S = (unsigned)S;
  a.slots_per_limb = (unsigned)spl;
  a.col0 = col0;
  a.logtot = a.logsub = logM;
  TabPtrs tp{};
  const T *srcs[3] = {A, Cc, B};
  T *dsts[3] = {W1, W3, W2};
  for (int k = 0; k < 3; k++) {
    a.W = dsts[k];
    a.src = srcs[k];
    launch_cross<false, CS_COSET, M>(ctx, a, ncols, logB, cp, st);
    if (k < 2) launch_sub<0, M>(ctx, dsts[k], ncols, col0, logM, logM, logB, nullptr, 1, S, spl, cp, st);
  }
  for (int i = limb0; i < ctx->L; i++) tp.t[i - limb0] = P->limb[i].d_cos_z;
  tp.w1 = W1;
  tp.w3 = W3;
  launch_sub<4, M>(ctx, W2, ncols, col0, logM, logM, logB, &tp, Mlen >> logB, S, spl, cp, st);
  a.W = W2;
  a.dst = H;
  if (!d1) {
    launch_cross<true, CD_H_COSET_CANON, M>(ctx, a, ncols, logB, cp, st);
    return;
  }
  launch_cross<true, CD_H_COSET, M>(ctx, a, ncols, logB, cp, st);
  launch_h_patch<M>(ctx, P, cp, H, A, B, ncols, col0, S, spl, d1, d2, d3, cm, st);
}

// the ZK patch of an H left in columns (h_patch_kernel), for this path and for the block convolutions
template <class M>
void launch_h_patch(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *H, const typename ArithOf<M>::T *A,
                    const typename ArithOf<M>::T *B, size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2,
                    const uint64_t *d3, const ColMap &cm, hipStream_t st) {
  const int logM = P->logM;
  const size_t Mlen = P->M;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((ncols * Mlen + 255) / 256, 256 * 16));
  ProfScope prof(ctx, st, "h_patch_kernel", (double)ncols * (double)Mlen * (d1 ? 32.0 : 16.0), d1 ? 24.0 * (double)ncols * (double)Mlen : 0.0);
  hipLaunchKernelGGL(h_patch_kernel<ColPlansT<M>>, dim3(blocks), dim3(256), 0, st, H, A, B, logM, (int)P->m, ncols, col0, (unsigned)S,
                     (unsigned)spl, cp, d1, d2, d3, cm);
  RS_HIP(hipGetLastError());
}

size_t big_chunk_cols(const WitnessPlan *P) {
  // two [cols][2M] workspaces within ~6 GiB
  const size_t per_col = 4 * P->M * sizeof(double);
  return std::max<size_t>(1, ((size_t)g_tune.witness_big_ws_mib << 20) / per_col);
}

#define RS_INSTANTIATE(M)                                                                                                                  \
  template bool tree_fwd_stages<M>(const WitnessPlan *);                                                                                   \
  template void big_interp<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, ArithOf<M>::T *, ArithOf<M>::T *, size_t, size_t, size_t, \
                              size_t, int, hipStream_t, int, bool);                                                                        \
  template void big_h<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, const ArithOf<M>::T *, const ArithOf<M>::T *, ArithOf<M>::T *, \
                         ArithOf<M>::T *, ArithOf<M>::T *, size_t, size_t, size_t, size_t, const uint64_t *, const uint64_t *,             \
                         const uint64_t *, const ColMap &, int, hipStream_t);                                                              \
  template void big_h_coset<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, const ArithOf<M>::T *, const ArithOf<M>::T *,          \
                               const ArithOf<M>::T *, ArithOf<M>::T *, ArithOf<M>::T *, ArithOf<M>::T *, size_t, size_t, size_t, size_t,   \
                               const uint64_t *, const uint64_t *, const uint64_t *, const ColMap &, int, hipStream_t);                    \
  template void launch_h_patch<M>(rs_ctx *, const WitnessPlan *, const ColPlansT<M> &, ArithOf<M>::T *, const ArithOf<M>::T *,             \
                                  const ArithOf<M>::T *, size_t, size_t, size_t, size_t, const uint64_t *, const uint64_t *,               \
                                  const uint64_t *, const ColMap &, hipStream_t);
RS_INSTANTIATE(Mod)
RS_INSTANTIATE(ModI)
#undef RS_INSTANTIATE

}  // namespace rs
