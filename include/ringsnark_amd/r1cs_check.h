/* ringsnark_amd/r1cs_check.h -- C ABI of the R1CS satisfaction check of librs_hip.so, present when rs_version() >= 102
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 this header).
 * Conventions as in ringsnark_amd.h, which this header includes: d_* device pointers, h_* host pointers, status codes,
 * rs_last_error.  Declared beside ringsnark_amd.h, like tuning.h: where oracle/_ref cannot be recompiled (no reference at
 * hand; oracle/Makefile then keeps the prebuilt one), tests/test_cabi.py accepts only the ringsnark_amd.h and ring.hpp that the
 * prebuilt binary was compiled from.
 *
 * r1cs_constraint_system::is_satisfied (relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:122-158): does
 * <a,(1,x)> * <b,(1,x)> == <c,(1,x)> hold for every constraint, in every slot of every limb -- and where not.  It is what
 * the reference asserts before proving (r1cs_to_qrp.tcc:156, groth16.tcc:74), i.e. the test of the PRECONDITION that
 * ringsnark_amd.h states for rs_witness_map (the coset form of H at multi-pass sizes) and that rs_groth16_prove and
 * rs_rinocchio_prove inherit without testing it: call it once per assignment, before them.
 * One fused kernel, one pass over the assignment, no [m][L][N] intermediate (DESIGN.md "R1CS satisfaction check").
 * d_assignment must hold ALL n_vars rows [n_vars][L][N] (primary then auxiliary, as for the provers).
 * Returns RS_OK whether or not the system is satisfied -- an unsatisfied assignment is an answer, not an error;
 * n_violated == 0 is the reference's `true`.  RS_ERR_INVALID for a null ctx, cs, d_assignment or h_report.
 * Every field is a function of the inputs only (no dependence on launch order).  Synchronises the stream. */
#ifndef RINGSNARK_AMD_R1CS_CHECK_H
#define RINGSNARK_AMD_R1CS_CHECK_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct rs_r1cs_report {
  uint64_t n_violated;   /* constraints with at least one (limb, slot) where <a,(1,x)> * <b,(1,x)> != <c,(1,x)> */
  uint64_t first_row;    /* lowest violated constraint index; m when n_violated == 0 */
  uint32_t first_limb;   /* with first_slot: the lowest ring-layout index limb*N + slot that violates first_row */
  uint32_t first_slot;
  uint64_t a, b, c;      /* canonical residues of the three evaluations at (first_row, first_limb, first_slot); 0 if none */
} rs_r1cs_report;
int rs_r1cs_check(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_assignment /* [n_vars][L][N], full */,
                  uint8_t *d_row_flags /* [m] or NULL: 1 = constraint violated in some slot */,
                  rs_r1cs_report *h_report, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
