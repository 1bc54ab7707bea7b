/* ringsnark_amd/bits.h -- C ABI of the bit decomposition of ring elements of librs_hip.so, present when rs_version() >= 109
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 keygen.h; 105 seeded.h; 106 batch.h; 107 r1cs_solve.h; 108 modswitch.h; 109 this header).  Conventions as in
 * ringsnark_amd.h, which this header includes: d_* device pointers, h_* host pointers, status codes, rs_last_error.
 * Declared beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * What pb_variable_array::fill_with_bits_of_field_element (gadgetlib/pb_variable.tcc:58-66, an empty stub) would have to
 * do for a ring element in NTT form, and what the reference's range-check circuit does by hand
 * (examples/example_plaintext_check_SEAL.cpp:72-80, benchmarks/bench_plaintext_check_SEAL.cpp:86-94): the wires b_k with
 * b_k * (1 - b_k) = 0 and x = sum_k 2^k b_k hold, slot by slot, the bits of the slot's value.  No constraint determines
 * them forwards, so rs_r1cs_solve (r1cs_solve.h) cannot produce them: a caller uploads x, calls this, marks the bit wires
 * as given, solves what is left, checks (r1cs_check.h) and proves.
 *
 * A slot's value is ONE integer v < 2^nbits, stored as the same word in every limb (v is a canonical residue of every
 * q_i because nbits <= floor(log2 q_i)).  Per (element, slot), with v the limb-0 word: bit row k holds (v >> k) & 1 at that
 * slot IN EVERY LIMB, k < nbits -- pure 0/1 rows.  Integers only, no modular arithmetic.
 *
 * LAYOUT.  Element e is the ring element [L][N] at d_x + e * x_stride * L*N; its bit k is written to the ring element at
 * d_bits + (e * bits_stride + k) * L*N; the strides count ring elements.  Rows between the bit rows are not touched.  With
 * x_stride = bits_stride = nbits + 1, d_bits = assignment + first_bit_row * L*N and d_x = d_bits + nbits * L*N the call
 * fills the blocks (b_0 .. b_{nbits-1}, x) of an assignment in place.
 *
 * BAD INPUT is an answer, not an error (as in r1cs_check.h and verify.h): RS_OK and a report.  A ring-layout position
 * (element, limb i, slot) is bad when i == 0 and v >= 2^nbits, or when i > 0 and the limb-i word differs from v.  The bits
 * written for a bad slot are the low nbits bits of v, so the packing constraint x = sum 2^k b_k then fails in rs_r1cs_check.
 * Every report field is a function of the inputs only (no dependence on launch order); clean input issues no atomic.
 *
 * RS_ERR_INVALID, with nothing written, for: a null context; count > 0 with a null d_x or d_bits; nbits outside
 * 1 .. min_i floor(log2 q_i); x_stride < 1; bits_stride < nbits; a pointer that is not 16-byte aligned; an extent that does
 * not fit the address space; an input row that shares a word with an output row (tested exactly, on the host, in
 * O(count), before anything is launched).  count == 0: RS_OK, nothing is done (a report is zeroed).
 * h_report == NULL: the work is enqueued on the stream and the call returns without a download or a synchronisation;
 * otherwise it synchronises the stream. */
#ifndef RINGSNARK_AMD_BITS_H
#define RINGSNARK_AMD_BITS_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct rs_bits_report {
  uint64_t n_bad;       /* ring-layout positions (element, limb, slot) that are bad */
  uint64_t first_elem;  /* lowest element with a bad position, then the lowest limb*N + slot in it; all 0 if n_bad == 0 */
  uint32_t first_limb, first_slot;
  uint64_t word, value; /* the word at that position; the limb-0 word of that slot */
} rs_bits_report;

int rs_ring_bit_decompose(rs_ctx *ctx, const uint64_t *d_x, size_t x_stride, size_t count, int nbits, uint64_t *d_bits,
                          size_t bits_stride, rs_bits_report *h_report, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
