// witness_plan.hpp -- the per-(context, m) plan of the witness map: the device tables of every limb (built by witness_plan.hip)
#pragma once
#include "rs_internal.hpp"

namespace rs {

// Device tables of one limb: arrays of 8-byte TABLE CONSTANTS of the context's arithmetic (balanced doubles for
// the FP64 arithmetic, Montgomery-form integers for the integer one; the zero constant is the zero word in both).
struct LimbPlan {
  uint64_t p = 0;
  void *d_tw = nullptr, *d_itw = nullptr;  // cyclic tables, 2M entries
  void *d_invfact = nullptr;               // [M]  1/j! (0 for j >= m)
  void *d_ehat = nullptr;                  // [2M] spectrum of (-1)^k/k!, scaled by 1/(2M)
  void *d_dhat = nullptr;                  // [logM+1][M] spectra of D_left per level, scaled by 1/n
  void *d_dlow = nullptr;                  // [SCHOOL_LEVELS+1][M/2] low coefficients of D_left
  void *d_shat = nullptr;                  // [2M] spectrum of rev(Z)^-1 mod x^(m-1), scaled 1/(2M)^2
  void *d_ztab = nullptr;                  // [M] Z_k (0 beyond m)
  // coset form of H (big_h_coset; full-length plans): g^k; g^-k / M; 1 / Z(g w^i) in the forward transform's output order
  void *d_cos_g = nullptr, *d_cos_h = nullptr, *d_cos_z = nullptr;  // [M] each
  // block-convolution path (WitnessPlan::bcLog != 0): spectra of the B-coefficient blocks of the same polynomials,
  // transform length 2B = 2^bcLog, scaled by 1/(2B)
  void *d_bc_e = nullptr;                  // [M/B][2B] blocks of (-1)^k/k!
  void *d_bc_s = nullptr;                  // [M/B][2B] blocks of rev(Z)^-1 mod x^(m-1)
  void *d_bc_d = nullptr;                  // [logM - bcLog][M] per level l > bcLog: [node][block][2B] blocks of D_left's low part
  // two-dimensional form of the same tables (WitnessPlan::bc2): per spectrum point, the Y-point transform ACROSS the
  // zero-padded sequence of blocks (Y = 2 x blocks of the operand), scaled by 1/(2B Y):
  void *d_b2_e = nullptr, *d_b2_s = nullptr;  // [Y][2B], Y = 2M/B
  void *d_b2_d = nullptr;                     // [logM - bcLog][2M]: per level l, [node][Y_l][2B], Y_l = 2^l / B
  uint32_t fwd_mask2 = 0, inv_mask2 = 0;     // reduce masks for length 2M
  int adic = 64;                             // incomplete transforms (WitnessPlan::incomplete): d_tw / d_itw hold 2^adic entries and
                                             // every spectrum table of a longer transform is in the incomplete form (witness_inc.hpp)
  std::vector<uint64_t> Z;                   // m+1 coefficients of the vanishing polynomial
};

struct WitnessPlan {
  size_t m = 0, M = 0;
  int logM = 0;
  // 0: every ring prime has a 2M-th root of unity (q = 1 mod 2M): full-length transforms.  Otherwise the largest
  // transform length every prime supports is 2^bcLog < 2M (capped at 2^13, one LDS tile) and every product longer
  // than that is a BLOCK convolution over blocks of B = 2^(bcLog-1) coefficients (see "block convolutions" below):
  // what makes the witness map work for the primes the reference's own recipe produces, which only guarantee
  // q = 1 mod 2*N_inner (seal/seal_util.hpp:20-32).
  int bcLog = 0;
  // Block convolutions as TWO-DIMENSIONAL transforms (FP64 arithmetic, primes with 2-adicity >= 14, M >= 2^15; see
  // "two-dimensional block convolutions" below): blocks of B = 2^13 coefficients, bcLog = 14.
  bool bc2 = false;
  // Some ring prime lacks a 2M-th root of unity and the columns take the multi-pass path with INCOMPLETE transforms
  // (witness_inc.hpp; LimbPlan::adic per prime) instead of block convolutions: bcLog = 0, the full-length launch sequences run.
  bool incomplete = false;
  std::vector<LimbPlan> limb;
  // coefficients_for_Z of every limb as the compact [m + 1][L] device array the inner products take a slot-constant
  // vector in (rs_msm_vec::slot_const): a per-(context, m) constant, uploaded once (witness_Z_rows)
  uint64_t *d_Zt = nullptr;
};

}  // namespace rs
