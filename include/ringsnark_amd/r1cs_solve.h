/* ringsnark_amd/r1cs_solve.h -- C ABI of the assignment solver of librs_hip.so, present when rs_version() >= 107
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 keygen.h; 105 seeded.h; 106 batch.h; 107 this header).  Conventions as in ringsnark_amd.h, which this header
 * includes: d_* device pointers, h_* host pointers, status codes, rs_last_error.  Declared beside ringsnark_amd.h for the
 * reason given in r1cs_check.h.
 *
 * The step BEFORE rs_r1cs_check and the provers: the full assignment [n_vars][L][N] from the wires the caller has.
 * Variables are numbered from 0 as the rows of the assignment are (variable v is column v + 1 of the matrices; column 0
 * is the constant one, always known).  The caller marks any subset of the variables as given.  Constraint j is READY
 * when every wire of its a and b rows is known, its c row holds exactly one distinct unknown wire w, w does not occur
 * in a or b, every c-row entry on w has a slot-constant scalar coefficient, and the sum k of those coefficients is
 * non-zero modulo every q_l.  It then determines, per limb and slot,
 *     w = (<a,(1,x)> * <b,(1,x)> - <c,(1,x)> without w) * k^-1        (a canonical residue).
 * Nothing else is solved: unknowns on the a / b side (inverse and division witnesses), polynomial coefficients on the
 * target -- such wires stay unsolved and are REPORTED (bit, inverse and quotient wires as declared hints of a plan: the
 * entry points of solve_hints.h).  The arithmetic is exact: every order of evaluation gives the same
 * words.
 *
 * The schedule (host, once per system and mask, O(nnz)): given wires have level 0; a step's level is 1 + the highest
 * level among the wires its constraint reads; a wire is determined in the lowest level in which some constraint for it
 * is ready and, within that level, by the lowest such constraint; steps are ordered by (level, constraint).  A
 * constraint whose wires are all known when it is reached determines nothing: it is left to rs_r1cs_check. */
#ifndef RINGSNARK_AMD_R1CS_SOLVE_H
#define RINGSNARK_AMD_R1CS_SOLVE_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct rs_r1cs_solve_plan rs_r1cs_solve_plan;
typedef struct rs_r1cs_solve_info {
  uint64_t n_given, n_solved, n_unsolved;
  uint64_t first_unsolved;   /* lowest 0-based variable neither given nor solved; n_vars if none */
  uint64_t n_levels, max_width;
  uint64_t n_unused;         /* constraints that determine nothing (checks, or never ready) */
  uint64_t first_blocked;    /* lowest constraint never ready that still holds an unknown wire; m if none */
  uint32_t blocked_reason;   /* of first_blocked, in the final state.  0 none; 1 unknown in a or b; 2 several unknowns in c;
                                3 polynomial coefficient on the target; 4 coefficient sum 0 modulo some q_l; 5 target also
                                in a or b (the only unknown of a and b is the only unknown of c) */
} rs_r1cs_solve_info;
/* A plan with unsolved wires is still a plan: RS_OK, and *h_info says what is missing and why.  The plan owns its device
 * arrays (step rows, target wires, k^-1 per limb as constants of the context's arithmetic) and takes no workspace slot.
 * It is bound to ctx and cs; cs must outlive it.  Reusable for every assignment, on any stream.  h_given: n_vars bytes,
 * non-zero = given.  h_info may be NULL. */
int rs_r1cs_solve_plan_create(rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given /* [n_vars] */, rs_r1cs_solve_plan **out,
                              rs_r1cs_solve_info *h_info);
/* The steps in order: constraint and 0-based target variable of each, and where every level starts.  Any pointer may be NULL. */
int rs_r1cs_solve_plan_steps(const rs_r1cs_solve_plan *plan, uint32_t *h_rows, uint32_t *h_wires /* [n_solved] each */,
                             uint64_t *h_level_ptr /* [n_levels + 1] */);
void rs_r1cs_solve_plan_destroy(rs_r1cs_solve_plan *plan);
/* The three modes produce identical words; LEVELS and WALK exist so that tests can drive each kernel. */
#define RS_SOLVE_AUTO 0
#define RS_SOLVE_LEVELS 1   /* one launch per level */
#define RS_SOLVE_WALK 2     /* one launch walks every step */
typedef struct rs_r1cs_solve_stats { uint32_t level_launches, walk_launches; } rs_r1cs_solve_stats;
/* Writes exactly the rows of the solved wires.  Never reads a row that is neither given nor already solved (such rows may
 * hold any bytes) and leaves the rows of unsolved wires untouched.  Given rows must be canonical.  Asynchronous on
 * `stream`.  RS_ERR_INVALID for a null ctx, plan or d_assignment, a plan of another context, or an unknown mode. */
int rs_r1cs_solve(rs_ctx *ctx, const rs_r1cs_solve_plan *plan, uint64_t *d_assignment /* [n_vars][L][N], in/out */, int mode,
                  rs_r1cs_solve_stats *h_stats /* or NULL */, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
