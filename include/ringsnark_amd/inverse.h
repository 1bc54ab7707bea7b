/* ringsnark_amd/inverse.h -- C ABI of the slotwise inverse-or-zero of ring elements of librs_hip.so, present when
 * rs_version() >= 113 (versions: 100 .. 109 as listed in bits.h; 110 verify_batch.h; 111 packed.h; 112 r1cs_batch.h; 113 this
 * header).  Conventions as in ringsnark_amd.h, which this header includes: d_* device pointers, h_* host pointers, status
 * codes, rs_last_error.  Declared beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * A ring element in evaluation form is L*N independent residues.  The inverse-or-zero of a wire x holds, slot by slot,
 * x^-1 where the slot is non-zero and 0 where it is zero: the witness of the is-zero gadget (x * inv = 1 - z, x * z = 0), of
 * every "x != 0" and "x = y" statement built on it, and -- with a numerator -- of every quotient wire y * b = a.  These wires
 * are determined through the a or b side of a constraint, so rs_r1cs_solve (r1cs_solve.h) cannot produce them: a caller
 * uploads x, calls this, marks the filled wires as given, solves what is left, checks (r1cs_check.h) and proves -- the flow
 * of bits.h.  rs_ring_inv (ringsnark_amd.h) refuses an element with a single zero slot and is unchanged.
 *
 * POSITIONS are (element e, limb i, slot s).  The strides count ring elements as in bits.h: element e of x is the ring
 * element [L][N] at d_x + e * x_stride * L*N, likewise for num and out.  Rows outside the output rows are not touched.
 *   0 < x < q_i                        out = x^-1 mod q_i (d_num == NULL) or num * x^-1 mod q_i: canonical residues
 *   x == 0                             out = 0; the position counts in n_zero
 *   x >= q_i, or num >= q_i (given)    out = 0; the position counts in n_bad and not in n_zero
 * Exact: out equals pow(x, q_i - 2, q_i) word for word, and rs_ring_inv wherever that call succeeds.
 *
 * ZEROS AND BAD WORDS are an answer, not an error (as in bits.h, r1cs_check.h and verify.h): RS_OK and a report.  Every
 * report field is a function of the inputs only (no dependence on launch order); input with no zero and no bad word issues
 * no atomic.
 *
 * RS_ERR_INVALID, with nothing written, for: a null context; count > 0 with a null d_x or d_out; a stride below 1
 * (num_stride only when d_num is given); a pointer that is not 16-byte aligned; an extent beyond 2^60 words; an input row,
 * of x or of num, that shares a word with an output row (tested exactly, on the host, in O(count), before anything is
 * launched).  Rows of x and rows of num may overlap each other or be the same: num = x yields the non-zero indicator 1 - z.
 * count == 0: RS_OK, nothing is done (a report is zeroed).  h_report == NULL: the work is enqueued on the stream and the call
 * returns without a download or a synchronisation; otherwise it synchronises the stream. */
#ifndef RINGSNARK_AMD_INVERSE_H
#define RINGSNARK_AMD_INVERSE_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct rs_inv_report {
  uint64_t n_zero;      /* positions (element, limb, slot) whose x word is 0 */
  uint64_t zero_elem;   /* the first of them: lowest element, then lowest limb*N + slot; all 0 if n_zero == 0 */
  uint32_t zero_limb, zero_slot;
  uint64_t n_bad;       /* positions whose x word, or num word when d_num is given, is >= q_limb (not a canonical residue) */
  uint64_t bad_elem;    /* the first of them, same order; all 0 if n_bad == 0 */
  uint32_t bad_limb, bad_slot;
  uint64_t bad_x, bad_num; /* the x word and the num word there (bad_num 0 when d_num == NULL) */
} rs_inv_report;        /* 64 bytes */

int rs_ring_inv_or_zero(rs_ctx *ctx, const uint64_t *d_x, size_t x_stride, const uint64_t *d_num, size_t num_stride,
                        size_t count, uint64_t *d_out, size_t out_stride, rs_inv_report *h_report, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
