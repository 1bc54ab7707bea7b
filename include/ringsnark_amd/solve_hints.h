/* ringsnark_amd/solve_hints.h -- C ABI of the assignment solver WITH HINTS of librs_hip.so, present when
 * rs_version() >= 114 (versions: 100 .. 113 as listed in inverse.h; 114 this header).  Conventions as in ringsnark_amd.h:
 * d_* device pointers, h_* host pointers, status codes, rs_last_error.  Declared beside ringsnark_amd.h for the reason
 * given in r1cs_check.h.
 *
 * rs_r1cs_solve (r1cs_solve.h) determines a wire only through the c side of a constraint.  Bit rows (bits.h), inverse-or-zero
 * wires and quotients (inverse.h) are determined through a or b; as stand-alone fills they serve only where their source is
 * an input.  A HINT declares such wires of ANY wire, the solver's own included: one plan from the system, the given mask and
 * the hints, and one call fills every wire that the constraints and the hints determine together.
 *
 * A hint (0-based variables, as the rows of the assignment):
 *   RS_HINT_BITS   variable dst + k * dst_stride  <-  (v >> k) & 1, k < nbits, in every limb, v the LIMB-0 word of src's slot
 *                  (bits.h semantics).  A position (hint, limb i, slot) is BAD when i == 0 and v >= 2^nbits, or i > 0 and
 *                  the limb-i word of src differs from v; the low nbits bits of v are written all the same.
 *   RS_HINT_INV    variable dst  <-  src^-1 per limb and slot, 0 where src is 0 (inverse.h semantics)
 *   RS_HINT_QUOT   variable dst  <-  num * src^-1, 0 where src is 0
 * num is read by QUOT only; nbits and dst_stride by BITS only.  Source rows are canonical residues: they are given rows,
 * which must be canonical, or rows the solver stored.
 *
 * THE SCHEDULE is that of r1cs_solve.h with these additions (host, once per system, mask and hint list, O(nnz + targets)):
 *   reservation  the targets of every declared hint are reserved: no constraint step ever determines one, and for the
 *                constraint counters a reserved wire is an unknown until its hint has run
 *   readiness    a hint is ready when src, and num for QUOT, are known
 *   levels       a hint's level is 1 + the highest level of its sources; it runs in the lowest level at which it is ready
 *   order        steps are ordered by level, then constraint steps by row, then hint steps by hint index; a level reads
 *                only lower levels
 * A cycle across hints is no error: those hints never become ready and are reported.  With n_hints == 0 the steps, level
 * pointers and info equal those of rs_r1cs_solve_plan_create field for field, and the solved words those of rs_r1cs_solve.
 *
 * RS_ERR_INVALID, before anything is allocated on the device, for: an unknown kind; src, num (QUOT) or a target out of
 * range; nbits outside 1 .. min_i floor(log2 q_i) or dst_stride < 1 (BITS); a target that is given; a target named twice, in
 * one hint or across hints; src or num among the hint's own targets.
 *
 * BAD BITS AND ZERO SOURCES are answers, not errors (as in bits.h and inverse.h): RS_OK and a report; rs_r1cs_check then
 * fails where the circuit forbids them.  Every report field is a function of the inputs only; clean input issues no atomic. */
#ifndef RINGSNARK_AMD_SOLVE_HINTS_H
#define RINGSNARK_AMD_SOLVE_HINTS_H
#include "r1cs_solve.h"
#ifdef __cplusplus
extern "C" {
#endif
#define RS_HINT_BITS 1
#define RS_HINT_INV 2
#define RS_HINT_QUOT 3
typedef struct rs_solve_hint { uint32_t kind, src, num, dst, nbits, dst_stride; } rs_solve_hint;

typedef struct rs_r1cs_hint_plan rs_r1cs_hint_plan;
typedef struct rs_r1cs_hint_info {
  rs_r1cs_solve_info solve;    /* the fields of r1cs_solve.h with their meanings.  n_solved counts WIRES, from constraints and
                                  hints alike; max_width counts the steps of a level; n_unused: constraints that are no step;
                                  blocked_reason 6: the only unknown is reserved for a hint that never became ready */
  uint64_t n_steps;            /* constraint steps + hint steps (n_solved when no BITS hint ran) */
  uint64_t n_hints_run, n_hints_blocked;
  uint64_t first_blocked_hint; /* lowest hint that never became ready; n_hints if none */
} rs_r1cs_hint_info;
/* As rs_r1cs_solve_plan_create; h_hints: n_hints hints, copied (NULL when n_hints == 0).  A plan with unsolved wires or
 * blocked hints is still a plan.  The plan owns its device arrays, the words of its report among them. */
int rs_r1cs_hint_plan_create(rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given /* [n_vars] */, const rs_solve_hint *h_hints,
                             size_t n_hints, rs_r1cs_hint_plan **out, rs_r1cs_hint_info *h_info);
/* The steps in order, [n_steps] each.  Kind 0 is a constraint step: index is the row, wire the target.  Kind 1 is a hint
 * step: index is the hint, wire its first target.  Any pointer may be NULL. */
int rs_r1cs_hint_plan_steps(const rs_r1cs_hint_plan *plan, uint8_t *h_kind, uint32_t *h_index, uint32_t *h_wire,
                            uint64_t *h_level_ptr /* [n_levels + 1] */);
void rs_r1cs_hint_plan_destroy(rs_r1cs_hint_plan *plan);

typedef struct rs_r1cs_hint_stats { uint32_t level_launches, walk_launches, hint_launches; } rs_r1cs_hint_stats;
typedef struct rs_solve_hint_report {
  uint64_t n_bits_bad;                      /* bad positions (hint, limb, slot) of BITS hints */
  uint32_t bad_hint, bad_limb, bad_slot;    /* the first: lowest hint, then lowest limb*N + slot; all 0 if none */
  uint32_t reserved0;
  uint64_t n_zero;                          /* positions of INV and QUOT hints whose src word is 0 */
  uint32_t zero_hint, zero_limb, zero_slot; /* the first of them, same order; all 0 if none */
  uint32_t reserved1;
} rs_solve_hint_report;                     /* 48 bytes */
/* rs_r1cs_solve with the hint steps: modes and guarantees as there (exactly the rows of the solved wires are written, no row
 * that is neither given nor solved is read).  The kernels: the level and walk kernels of r1cs_solve.h for constraint steps, a
 * hint-level kernel for the hint steps of one level, and a walk kernel that runs INV and QUOT hint steps inline (they are
 * slot-local).  A BITS hint step is not slot-local -- limb i needs the limb-0 word, which another workgroup stored -- so in
 * EVERY mode, RS_SOLVE_WALK included, it ends a walk run and goes to the hint-level kernel.  A plan whose levels hold no
 * hint steps launches exactly what rs_r1cs_solve launches.
 * h_report == NULL: enqueued only.  Otherwise the call synchronises the stream.  The plan owns the report words on the
 * device: two calls on one plan that both take a report must not overlap. */
int rs_r1cs_solve_hinted(rs_ctx *ctx, const rs_r1cs_hint_plan *plan, uint64_t *d_assignment /* [n_vars][L][N], in/out */, int mode,
                         rs_r1cs_hint_stats *h_stats /* or NULL */, rs_solve_hint_report *h_report /* or NULL */, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
