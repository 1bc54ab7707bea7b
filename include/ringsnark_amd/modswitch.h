/* ringsnark_amd/modswitch.h -- C ABI of MOD-SWITCHED encodings and proofs of librs_hip.so, present when rs_version() >= 108.
 * Conventions as in ringsnark_amd.h and verify.h, which this header includes.
 *
 * EncodingElem::modswitch_inplace (ringsnark/seal/seal_ring.hpp:370, seal_ring.tcc:317-322) calls SEAL's
 * mod_switch_to_next_inplace on each of the L ciphertexts of an element.  SEAL is not vendored; the arithmetic is that of
 * SEAL 4.x BGV mod_t_and_divide_q_last_ntt_inplace, recalled here.  One step K_in -> K_in - 1 works per (element, limb i,
 * component c) with t = q_i and p = Q[K_in - 1]:
 *   1. last = iNTT_p(row K_in - 1), canonical in [0, p)
 *   2. u    = (-last * p^-1) mod t, canonical in [0, t)
 *   3. for each j < K_in - 1:  delta_j = NTT_{Q_j}((last + u * p) mod Q_j),   c'_j = (c_j - delta_j) * p^-1 mod Q_j
 * and K_in -> K_out is K_in - K_out such steps in sequence.  The result is an ordinary ciphertext of the context with the
 * truncated prime list Q[:K_out] -- canonical, NTT form, compact layout [count][L][2][K_out][N_enc] -- that decrypts to
 * m * (prod_{j >= K_out} Q_j)^-1 mod t.  A decode at level K_lvl therefore multiplies by
 *     F_i = prod_{j >= K_lvl} Q_j mod q_i
 * after the centred reduction (SEAL's correction_factor; here a function of the context and the level, so it never travels).
 * Noise of one step: |v'| < |v| / p + t * (1 + N_enc * |s|_inf).
 *
 * A LEVEL K_lvl, 1 <= K_lvl <= K, names the first K_lvl primes of the context; level K is an unswitched encoding.  Every call
 * returns RS_ERR_INVALID for a level outside that range.  The prover needs no secret to switch, chooses the level, and the
 * verifier's noise guard decides whether it was too low (RS_ERR_NOISE). */
#ifndef RINGSNARK_AMD_MODSWITCH_H
#define RINGSNARK_AMD_MODSWITCH_H
#include "verify.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_in [count][L][2][K_in][N_enc] -> d_out [count][L][2][K_out][N_enc], 1 <= K_out <= K_in <= K.  Out of place: ranges that
 * overlap return RS_ERR_INVALID.  K_out == K_in is a copy.  Input words must be canonical residues of their primes (they
 * need not form valid ciphertexts).  The intermediate levels of a switch of several steps live in the context's workspace.
 * Asynchronous on `stream`. */
int rs_enc_mod_switch(rs_ctx *ctx, const uint64_t *d_in, size_t count, int K_in, int K_out, uint64_t *d_out, rs_stream stream);

/* rs_enc_decode / rs_enc_noise_budget at a level: d_sk [K][N_enc] as everywhere (its first K_lvl rows are read), d_enc
 * [count][L][2][K_lvl][N_enc].  The decode of the context with primes Q[:K_lvl] -- its CRT constants, floor(Q/2) digits and
 * threshold table, built at the first call of a level and kept in the context -- times F_i.  The noise guard and its message
 * are those of rs_enc_decode.  K_lvl == K gives the words of rs_enc_decode and rs_enc_noise_budget.  Synchronise. */
int rs_enc_decode_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings,
                        rs_stream stream);
int rs_enc_noise_budget_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, int *h_budget,
                              rs_stream stream);

/* The wire format "RSNKENC1" of ringsnark_amd.h with K = K_lvl and Q[:K_lvl] in the header and K_lvl rows per component:
 * byte for byte what a context created on the truncated prime list writes.  rs_enc_wire_size_level returns 0 for a null
 * context or a level out of range.  rs_enc_deserialize_level accepts a stream of any level of the context (any prefix of its
 * primes), reports the level in *h_K_lvl and checks every residue against that level's primes; d_enc == NULL is the size and
 * level query; capacity counts elements of the level found. */
size_t rs_enc_wire_size_level(const rs_ctx *ctx, int K_lvl, size_t count);
int rs_enc_serialize_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_enc, const uint8_t *h_empty, size_t count, void *h_buf,
                           size_t buf_bytes, rs_stream stream);
int rs_enc_deserialize_level(rs_ctx *ctx, const void *h_buf, size_t buf_bytes, uint64_t *d_enc, uint8_t *h_empty, size_t capacity,
                             size_t *h_count, int *h_K_lvl, rs_stream stream);

/* rs_groth16_verify / rs_rinocchio_verify on a proof of level K_lvl: d_proof [3 | 9][L][2][K_lvl][N_enc].  Everything else,
 * h_empty and the report included, as in verify.h: for a level whose budget is not spent the report equals that of the
 * unswitched proof field for field. */
int rs_groth16_verify_level(rs_ctx *ctx, const rs_groth16_vk *vk, int K_lvl, const uint64_t *d_primary, const uint64_t *d_proof,
                            const int *h_empty /* [3] or NULL */, rs_verify_report *h_report, rs_stream stream);
int rs_rinocchio_verify_level(rs_ctx *ctx, const rs_rinocchio_vk *vk, int K_lvl, const uint64_t *d_primary, const uint64_t *d_proof,
                              const int *h_empty /* [9] or NULL */, rs_verify_report *h_report, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
