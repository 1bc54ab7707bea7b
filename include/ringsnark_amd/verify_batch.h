/* ringsnark_amd/verify_batch.h -- C ABI of BATCHED verification of librs_hip.so, present when rs_version() >= 110
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 keygen.h; 105 seeded.h; 106 batch.h; 107 r1cs_solve.h; 108 modswitch.h; 109 bits.h; 110 this header).  Conventions as
 * in ringsnark_amd.h, verify.h and modswitch.h, which this header includes.  Declared beside ringsnark_amd.h for the reason
 * given in r1cs_check.h.
 *
 * groth16::verifier (zk_proof_systems/groth16/groth16.tcc:117-170) and rinocchio::verifier
 * (zk_proof_systems/rinocchio/rinocchio.tcc:192-295) take one proof.  A verifier that holds one key and receives many
 * proofs calls them in a loop, and every call decodes three or nine elements (EncT::decode, seal_ring.tcc:435-477) and
 * recomputes the public sums from all 3 (n_inputs + 1) columns of the key.  These calls verify `batch` proofs of ONE key in
 * one pass: one decode of all the elements, and one check kernel in which a thread keeps the public sums of
 * several proofs (rs_verify_batch_group of them) in registers, so that a column of the key is read once per group of proofs.
 *
 * THE CONTRACT.  For every b, (h_status[b], h_reports[b]) is WORD FOR WORD what rs_groth16_verify_level /
 * rs_rinocchio_verify_level return for proof b alone with the same key, inputs and flags: RS_OK and the same
 * rs_verify_report in every field, or -- where the single call returns RS_ERR_NOISE -- h_status[b] = RS_ERR_NOISE and an
 * all-zero report (accepted = 0).  No field depends on launch order or on the other proofs of the batch.  The call itself
 * returns RS_OK whenever it ran, whatever the verdicts: a spent budget in one proof is an answer about that proof. */
#ifndef RINGSNARK_AMD_VERIFY_BATCH_H
#define RINGSNARK_AMD_VERIFY_BATCH_H
#include "modswitch.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RS_VERIFY_BATCH_MAX 64

/* Proofs whose public sums one thread of the check kernel carries in registers (a compile-time constant of the library;
 * batches need not be multiples of it). */
int rs_verify_batch_group(void);

/* K_lvl: the level of EVERY proof of the batch, 1 <= K_lvl <= K (K: unswitched proofs; modswitch.h), else RS_ERR_INVALID.
 * batch: 1..RS_VERIFY_BATCH_MAX; 0 returns RS_OK and writes nothing; negative or larger: RS_ERR_INVALID.
 * d_primary [batch][n_inputs][L][N] (may be NULL when n_inputs == 0); d_proofs [batch][3][L][2][K_lvl][N_enc];
 * h_empty [batch][3] or NULL: h_empty[3 b + k] != 0 marks element k of proof b EMPTY -- the zero ring element, its payload
 * is not read.  The runs of consecutive non-EMPTY elements of the flattened [batch * 3] sequence are decoded, so a batch
 * without EMPTY elements is one decode of 3 * batch elements.
 * h_status [batch]: RS_OK or RS_ERR_NOISE; h_reports [batch]; h_budget_min [batch] or NULL: the smallest
 * rs_enc_noise_budget_level value over the non-EMPTY ciphertexts (element x limb) of proof b, and for a proof whose
 * elements are all EMPTY bit_count(Q[0] .. Q[K_lvl - 1]) - 1, the budget of a ciphertext of that level whose noise
 * polynomial is zero (the largest value the budget can take).
 * A key of another context or of the other scheme, or a null argument: RS_ERR_INVALID, nothing written.
 * The decoded elements and the report words live in the context's workspace: calls on one context serialise, and the
 * key is only read.  Synchronises. */
int rs_groth16_verify_batch(rs_ctx *ctx, const rs_groth16_vk *vk, int K_lvl, int batch, const uint64_t *d_primary,
                            const uint64_t *d_proofs, const int *h_empty, int *h_status, int *h_budget_min,
                            rs_verify_report *h_reports, rs_stream stream);
/* The same for Rinocchio: d_proofs [batch][9][L][2][K_lvl][N_enc], h_empty [batch][9] or NULL.  Proof b with element 8
 * EMPTY skips check 4 for that proof only (rinocchio.tcc:199-206, 283-288). */
int rs_rinocchio_verify_batch(rs_ctx *ctx, const rs_rinocchio_vk *vk, int K_lvl, int batch, const uint64_t *d_primary,
                              const uint64_t *d_proofs, const int *h_empty, int *h_status, int *h_budget_min,
                              rs_verify_report *h_reports, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
