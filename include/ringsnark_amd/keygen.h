/* ringsnark_amd/keygen.h -- C ABI of the two generators of librs_hip.so, present when rs_version() >= 104
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 this header).  Conventions as in ringsnark_amd.h, which this header includes: d_* device pointers, h_* host pointers,
 * status codes, rs_last_error.  Declared beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * groth16::generator (zk_proof_systems/groth16/groth16.tcc:5-66) and rinocchio::generator
 * (zk_proof_systems/rinocchio/rinocchio.tcc:5-72): the PROVING KEY vectors that rs_groth16_pk / rs_rinocchio_pk hold, from the
 * trapdoor that rs_groth16_vk_create / rs_rinocchio_vk_create take.  Both start with
 * r1cs_to_qrp_instance_map_with_evaluation(cs, s) (groth16.tcc:7-9, rinocchio.tcc:7-9) -- the code behind
 * rs_instance_map_eval -- and encode ring elements that are linear forms of its rows:
 *     key[t] = E( sum_{r < R} coef_r * row_r[t] ),   R <= 3, coef_r ring elements computed once per call,
 * which one kernel evaluates, batch-encodes and encrypts per element (DESIGN.md section 3 "Generator": K + 1 transforms
 * per (element, limb)).  All arithmetic is exact and the ring is commutative: every residue equals the reference's, and
 * every vector equals rs_enc_encode of the same ring elements with the same seed, bit for bit.
 *
 * Out of scope, because no prover or verifier of this library reads them: the reference's gamma_io (groth16.tcc:42-50),
 * alpha_rv_ts / alpha_rw_ts / alpha_ry_ts and rv_vs / rw_ws / ry_ys (rinocchio.tcc:36-47).
 *
 * Randomness: as rs_enc_encode.  Vector v encodes its element k from the stream h_seeds[v] + k (splitmix64, ternary error:
 * the CPU oracle's recipe -- SEAL's Blake2xb / centred-binomial sampler is not restated, so ciphertext BYTES are not SEAL's;
 * the scheme and every decryption are).  Two elements that share a stream share `a` and `e`, and their difference reveals
 * the difference of their plaintexts: the calls return RS_ERR_INVALID when the ranges [h_seeds[v], h_seeds[v] + len_v)
 * (modulo 2^64) of two vectors intersect.
 *
 * Errors, all found before any output is written: RS_ERR_INVALID (null argument, a constraint system of another context,
 * intersecting seed ranges, N_enc > 16384 as in rs_enc_encode); RS_ERR_NOT_INVERTIBLE "element is not invertible in ring"
 * when delta is not a unit (groth16.tcc:21 divides by it); RS_ERR_NOT_INVERTIBLE "t cannot be one of the values in the
 * domain" when s is a domain element (the error of rs_instance_map_eval).
 *
 * Memory: the internals of rs_instance_map_eval are used as they are, so the peak is, in ring elements [L][N],
 *     m (Lagrange values) + (m + 1) (powers of s) + 3 * (n_vars + 1) (A_k(s), B_k(s), C_k(s)) + 8,
 * plus, for a host-resident key, two staging buffers of `tile` encoding elements -- computed, not measured: about 80 GiB
 * at 2^16 constraints of the headline shape.  Everything derived from the trapdoor (the Lagrange values, the rows, Z(s),
 * delta^-1 and the coefficient elements) is overwritten with zeros before it is released, as rs_*_vk_destroy does.
 * Both calls synchronise.
 *
 * Seeded keys -- the vectors stored as their c0 halves and a public seed, half the size -- are in seeded.h (rs_version() >= 105). */
#ifndef RINGSNARK_AMD_KEYGEN_H
#define RINGSNARK_AMD_KEYGEN_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Where groth16.hpp:22-48 proving_key goes: the pointers the caller later puts into rs_groth16_pk.
 *   s_pows[t]    = E(s^t), t <= m                                              (groth16.tcc:27-30, 58)
 *   delta_ts[t]  = E(s^t * Z(s) * delta^-1), t <= m                            (groth16.tcc:32-35, 60)
 *   delta_mid[i] = E((beta A_k(s) + alpha B_k(s) + C_k(s)) * delta^-1), k = n_inputs + 1 + i, i < n_aux = n_vars - n_inputs
 *                                                                              (groth16.tcc:52-55, 59)
 *   d_alpha, d_beta = E(alpha), E(beta)                                        (groth16.tcc:57)
 * ZERO-INITIALISE the struct. */
typedef struct rs_groth16_key_out {
  uint64_t *s_pows, *delta_ts; /* [m+1] encoding elements */
  uint64_t *delta_mid;         /* [n_aux]; may be NULL when n_aux == 0 */
  uint64_t *d_alpha, *d_beta;  /* one element each, always on the device */
  int host_key;                /* 1: the three vectors are HOST pointers (pinned memory recommended: rs_host_alloc) -- a key larger
                                * than HBM.  Tiles of `tile` elements are encoded into two device staging buffers and copied to the
                                * host on a stream of their own, the copy of tile k under the kernel of tile k + 1. */
  size_t tile;                 /* elements per staging buffer when host_key; 0 = default (64) */
} rs_groth16_key_out;
/* d_s, d_alpha, d_beta, d_delta [L][N]; d_sk [K][N_enc] in NTT form (as rs_enc_encode takes it).
 * h_seeds: s_pows, delta_ts, delta_mid, alpha, beta (lengths m + 1, m + 1, n_aux, 1, 1). */
int rs_groth16_keygen(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                      const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const rs_groth16_key_out *out,
                      rs_stream stream);

/* Where rinocchio.hpp:22-58 proving_key goes (the members rs_rinocchio_pk holds).
 *   s_pows[t]       = E(s^t), alpha_s_pows[t] = E(alpha * s^t), t <= m         (rinocchio.tcc:21-27, 48-49)
 *   beta_prods[i]   = E(beta * (r_v A_k(s) + r_w B_k(s) + r_y C_k(s))), k = n_inputs + 1 + i    (rinocchio.tcc:29-34, 50)
 *   d_beta_rv_ts    = E(beta * Z(s) * r_v), d_beta_rw_ts, d_beta_ry_ts likewise                 (rinocchio.tcc:51-53)
 * ZERO-INITIALISE the struct. */
typedef struct rs_rinocchio_key_out {
  uint64_t *s_pows, *alpha_s_pows;                    /* [m+1] */
  uint64_t *beta_prods;                               /* [n_aux]; may be NULL when n_aux == 0 */
  uint64_t *d_beta_rv_ts, *d_beta_rw_ts, *d_beta_ry_ts; /* one element each, always on the device */
  int host_key;                                       /* as in rs_groth16_key_out: s_pows, alpha_s_pows, beta_prods on the host */
  size_t tile;
} rs_rinocchio_key_out;
/* h_seeds: s_pows, alpha_s_pows, beta_prods, beta_rv_ts, beta_rw_ts, beta_ry_ts (lengths m + 1, m + 1, n_aux, 1, 1, 1). */
int rs_rinocchio_keygen(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                        const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                        const uint64_t h_seeds[6], const rs_rinocchio_key_out *out, rs_stream stream);

/* The kernel of the generators on its own: d_enc[k] = E(sum_{r < n_terms} d_coef[r] * d_rows[r][k]) for k < count, element k
 * from the stream seed + k.  d_rows[r]: [count][L][N]; d_coef[r]: one ring element [L][N] or NULL (= 1); 1 <= n_terms <= 3.
 * With n_terms = 1 and d_coef[0] = NULL it writes the bytes of rs_enc_encode(ctx, d_sk, d_rows[0], count, seed, d_enc).
 * Synchronises. */
int rs_enc_encode_linear(rs_ctx *ctx, const uint64_t *d_sk, const uint64_t *const *d_coef, const uint64_t *const *d_rows,
                         int n_terms, size_t count, uint64_t seed, uint64_t *d_enc, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
