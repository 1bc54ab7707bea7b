/* ringsnark_amd/r1cs_batch.h -- C ABI of the BATCHED assignment solver and satisfaction check of librs_hip.so, present when
 * rs_version() >= 112 (versions: 100 .. 111 as listed in verify_batch.h and packed.h; 112 this header).  Conventions as in
 * ringsnark_amd.h, batch.h, r1cs_solve.h and r1cs_check.h, which this header includes.  Declared beside ringsnark_amd.h for
 * the reason given in r1cs_check.h.
 *
 * The two steps in front of every proof, for the `batch` assignments that rs_*_prove_batch takes: the members of a batch
 * are independent problems on ONE schedule and ONE set of matrices, so one thread carries its slot pair of every member.
 * Every schedule word, row bound, column index, coefficient and polynomial-table word is read once per batch, there is one
 * launch per level or run (solve) and one main and one epilogue launch (check) where `batch` single calls take `batch`,
 * and a thread has `batch` independent assignment loads in flight where the single kernels have one.
 * 1 <= batch <= RS_MAX_BATCH (batch.h).  d_assignments: HOST array of `batch` device pointers, each [n_vars][L][N]. */
#ifndef RINGSNARK_AMD_R1CS_BATCH_H
#define RINGSNARK_AMD_R1CS_BATCH_H
#include "batch.h"
#include "r1cs_check.h"
#include "r1cs_solve.h"
#ifdef __cplusplus
extern "C" {
#endif
/* One plan -- one system, one given mask -- serves every member.  Member b's rows after the call are WORD FOR WORD what
 * rs_r1cs_solve(ctx, plan, d_assignments[b], mode, ...) writes (the arithmetic is exact), and every promise of r1cs_solve.h
 * holds per member: exactly the rows of the solved wires are written, no row that is neither given nor already solved is
 * read, unsolved rows stay untouched, the call is asynchronous on `stream`.  h_stats counts the launches of the WHOLE batch:
 * in every mode they equal those of one rs_r1cs_solve call on the same plan.
 * RS_ERR_INVALID, before anything is written: batch < 1 or batch > RS_MAX_BATCH; a null ctx, plan, d_assignments or member;
 * a plan of another context; an unknown mode; two members whose byte ranges [p, p + n_vars * L * N * 8) overlap. */
int rs_r1cs_solve_batch(rs_ctx *ctx, const rs_r1cs_solve_plan *plan, int batch, uint64_t *const *d_assignments, int mode,
                        rs_r1cs_solve_stats *h_stats /* or NULL */, rs_stream stream);
/* h_reports[b] equals field for field what rs_r1cs_check reports for member b, and row b of d_row_flags its flag bytes.  An
 * unsatisfied member is an answer, not an error, and changes nothing in any other member's report.  Members may alias (the
 * call only reads).  One download of `batch` reports; synchronises the stream once.
 * RS_ERR_INVALID: batch out of range, a null ctx, cs, d_assignments, member or h_reports, a system of another context. */
int rs_r1cs_check_batch(rs_ctx *ctx, const rs_r1cs *cs, int batch, const uint64_t *const *d_assignments,
                        uint8_t *d_row_flags /* [batch][m] or NULL */, rs_r1cs_report *h_reports /* [batch] */, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
