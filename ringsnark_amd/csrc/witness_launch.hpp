// witness_launch.hpp -- the host functions through which the units of the witness map call each other (witness.hip has the map).
// Plain functions, and templates on the arithmetic M alone: each of those is instantiated for Mod and ModI in the unit that
// defines it.  No kernel crosses a unit: every kernel template is instantiated by the launch code of exactly one unit.
#pragma once
#include "witness_cols.hpp"
#include "witness_plan.hpp"

namespace rs {

struct TabPtrs;  // witness_multipass.hpp

// ---- witness_plan.hip: the plan cache and the column plans
uint64_t konst_word(const rs_ctx *ctx, uint64_t v, uint64_t p);
bool single_tile_ok(int logM);
WitnessPlan *get_plan(rs_ctx *ctx, size_t m);
template <class M>
ColPlansT<M> make_colplans(rs_ctx *ctx, const WitnessPlan *P, int limb0 = 0);

// ---- witness_lds.hip: the product tree's tiles
double tree_fp64(double T, int logT, bool pw_reduce = true);
void launch_tree_tiles(rs_ctx *ctx, double *cols, size_t ncols, size_t col0, int logM, int logT, size_t S, size_t slots_per_limb,
                       const ColPlans &cp, hipStream_t st, bool newton = false, double *Wout = nullptr, int rf = 0);
template <class M>
void launch_tree_tiles_generic(rs_ctx *ctx, typename ArithOf<M>::T *cols, size_t ncols, size_t col0, int logM, int logT, size_t S,
                               size_t slots_per_limb, const ColPlansT<M> &cp, hipStream_t st);

// ---- witness_lds.hip: a whole column in one LDS tile
int col_threads(size_t M);
template <class M>
void launch_interp_columns(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *cols, size_t ncols, size_t S,
                           size_t slots_per_limb, hipStream_t st);
void launch_h_tile(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, const double *A, const double *B, double *H, size_t S, size_t spl,
                   const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, hipStream_t st);
template <class M>
void launch_h_columns(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A,
                      const typename ArithOf<M>::T *B, typename ArithOf<M>::T *H, size_t S, size_t spl, const uint64_t *d1,
                      const uint64_t *d2, const uint64_t *d3, const ColMap &cm, hipStream_t st);

// ---- witness_big.hip: the multi-pass path
template <class M>
bool tree_fwd_stages(const WitnessPlan *P);
template <class M>
void big_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *X, typename ArithOf<M>::T *W, size_t ncols,
                size_t col0, size_t S, size_t spl, int limb0, hipStream_t st, int phases = 7, bool tree_fwd = false);
template <class M>
void big_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A, const typename ArithOf<M>::T *B,
           typename ArithOf<M>::T *H, typename ArithOf<M>::T *W1, typename ArithOf<M>::T *W2, size_t ncols, size_t col0, size_t S, size_t spl,
           const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, int limb0, hipStream_t st);
template <class M>
void big_h_coset(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A, const typename ArithOf<M>::T *B,
                 const typename ArithOf<M>::T *Cc, typename ArithOf<M>::T *H, typename ArithOf<M>::T *W1, typename ArithOf<M>::T *W2,
                 size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm,
                 int limb0, hipStream_t st);
size_t big_chunk_cols(const WitnessPlan *P);
// two kernels of witness_multipass.hpp that the block convolutions (witness_lds.hip) launch as well
template <class M>
void launch_h_patch(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *H, const typename ArithOf<M>::T *A,
                    const typename ArithOf<M>::T *B, size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2,
                    const uint64_t *d3, const ColMap &cm, hipStream_t st);
void launch_sub_wide_bc2(int mode, double *Ws, const TabPtrs &tp, unsigned period, size_t col0, unsigned S, unsigned spl, const ColPlans &cp,
                         unsigned long long nb, const double *Wy, hipStream_t st);

// ---- witness_lds.hip: block convolutions, pairwise (bc_*) and two-dimensional (bc2_*, FP64 arithmetic)
template <class M>
void bc_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, typename ArithOf<M>::T *X, size_t ncols, size_t col0, size_t S,
               size_t spl, hipStream_t st);
template <class M>
void bc_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlansT<M> &cp, const typename ArithOf<M>::T *A, const typename ArithOf<M>::T *Bc,
          typename ArithOf<M>::T *H, size_t ncols, size_t col0, size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2,
          const uint64_t *d3, const ColMap &cm, hipStream_t st);
void bc2_interp(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, double *X, size_t ncols, size_t col0, size_t S, size_t spl, int limb0,
                hipStream_t st, int phases = 7);
void bc2_h(rs_ctx *ctx, const WitnessPlan *P, const ColPlans &cp, const double *A, const double *Bc, double *H, size_t ncols, size_t col0,
           size_t S, size_t spl, const uint64_t *d1, const uint64_t *d2, const uint64_t *d3, const ColMap &cm, int limb0, hipStream_t st);
size_t bc_chunk_cols(const WitnessPlan *P);
// ---- witness_lds.hip: the generic sub-transform kernel, for witness_big.hip
template <class M>
void launch_sub_generic(int mode, typename ArithOf<M>::T *X, size_t nblocks, int logB, int log_n1, const TabPtrs &tp, size_t tab_period,
                        size_t bpc, size_t col0, size_t S, size_t spl, const ColPlansT<M> &cp, size_t lds, hipStream_t st);

}  // namespace rs
