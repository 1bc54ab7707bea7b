/* ringsnark_amd/seeded.h -- C ABI of SEEDED proving keys of librs_hip.so, present when rs_version() >= 105
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 keygen.h; 105 this header).  Conventions as in ringsnark_amd.h and keygen.h, which this header includes.  Declared
 * beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * Half of every element of a proving key is a counter-based stream: the encoder writes
 *     c1_j[p] = draw (n + j n + p + 1) of the element's per-limb stream, % Q_j        (n = N_enc)
 * and c0 = -(c1 s + t e) + m.  A SEEDED key vector keeps the c0 halves and one 64-bit PUBLIC seed, and c1 is recomputed
 * where the key is used -- as SEAL ships symmetric ciphertexts (seeded ciphertexts).  Every key is half the size: in HBM,
 * in host memory, in the generator's copies to the host and on the host link a prover with a host-resident key waits on.
 *
 * Compact layout: a seeded vector is [count][L][K][N_enc] words, the c0 blocks of [count][L][2][K][N_enc] in their order.
 *
 * TWO SEEDS PER VECTOR.  keygen.h draws the error e (draws 1..n) and a = c1 (draws n + 1..) of an element from one stream.
 * Whoever knows that stream's seed computes e, and with one known plaintext -- s_pows[0] = E(1) -- solves
 * c0 = -(a s + t e) + m for the secret key.  A seeded vector therefore has a PUBLIC seed P that generates a only and goes
 * to the prover, and the PRIVATE seed of keygen.h that generates e and never leaves the generator:
 *     element k, limb l:  a_j[p] = draw (n + j n + p + 1) of the stream (P + k) * 1315423911 + l + 1, % Q_j;
 *                         e from the stream (S + k) * 1315423911 + l + 1 as before.
 * The derivation and indexing are those of rs_enc_encode, so P = S reproduces the bytes of keygen.h -- FOR TESTS ONLY (it
 * hands e to the prover).  The public ranges [P_v, P_v + len_v) of the vectors of one key must be disjoint modulo 2^64, like
 * the private ones: two elements that share a reveal the difference of their plaintexts.  The calls return RS_ERR_INVALID,
 * before anything is written, when two public ranges or two private ranges intersect.  splitmix64 is the CPU oracle's recipe,
 * not a cryptographic generator: the caveat of keygen.h "Randomness" holds here word for word. */
#ifndef RINGSNARK_AMD_SEEDED_H
#define RINGSNARK_AMD_SEEDED_H
#include "keygen.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The expansion kernel on its own: d_enc[i] (full format) for i < count from d_c0[i] (compact: d_c0 points at the FIRST of
 * the `count` elements), c0 copied, c1 regenerated from the stream of STORED index first + i of a vector with public seed
 * pub_seed.  Exact: c1 equals the words the encoder writes (z % Q_j computed as z - hi(z floor(2^64 / Q_j)) Q_j and two
 * conditional subtractions, exact for every Q_j < 2^62).  Pointers 16-byte aligned.  Asynchronous on `stream`. */
int rs_enc_expand_seeded(rs_ctx *ctx, const uint64_t *d_c0, uint64_t pub_seed, size_t first, size_t count, uint64_t *d_enc,
                         rs_stream stream);

/* rs_groth16_key_out with COMPACT vectors; d_alpha, d_beta stay full-format elements on the device (their c1 from their
 * public seed).  host_key, tile as there: the staging tiles and the copies to the host are half the size.
 * ZERO-INITIALISE the struct. */
typedef struct rs_groth16_seeded_key_out {
  uint64_t *s_pows, *delta_ts; /* [m+1][L][K][N_enc] */
  uint64_t *delta_mid;         /* [n_aux][L][K][N_enc]; may be NULL when n_aux == 0 */
  uint64_t *d_alpha, *d_beta;  /* one full element each, always on the device */
  int host_key;
  size_t tile;
} rs_groth16_seeded_key_out;
/* rs_groth16_keygen plus h_pub_seeds: the public seeds of s_pows, delta_ts, delta_mid, alpha, beta. */
int rs_groth16_keygen_seeded(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                             const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const uint64_t h_pub_seeds[5],
                             const rs_groth16_seeded_key_out *out, rs_stream stream);

typedef struct rs_rinocchio_seeded_key_out {
  uint64_t *s_pows, *alpha_s_pows;                      /* [m+1][L][K][N_enc] */
  uint64_t *beta_prods;                                 /* [n_aux][L][K][N_enc]; may be NULL when n_aux == 0 */
  uint64_t *d_beta_rv_ts, *d_beta_rw_ts, *d_beta_ry_ts; /* one full element each, always on the device */
  int host_key;
  size_t tile;
} rs_rinocchio_seeded_key_out;
/* h_pub_seeds: s_pows, alpha_s_pows, beta_prods, beta_rv_ts, beta_rw_ts, beta_ry_ts. */
int rs_rinocchio_keygen_seeded(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                               const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                               const uint64_t h_seeds[6], const uint64_t h_pub_seeds[6], const rs_rinocchio_seeded_key_out *out,
                               rs_stream stream);

/* rs_msm / rs_msm_hostkey over COMPACT key vectors: crs[c] has public seed h_pub_seeds[c]; crs_on_host: 0 = device
 * pointers, 1 = host pointers (pinned memory recommended; the call then synchronises like rs_msm_hostkey).  crs_window as in
 * rs_msm: logical element t is STORED element t % crs_window and is regenerated with that stored index.
 * The term tiles (at most the tuning knob msm_host_tile elements per vector, for a device-resident key too) are expanded by
 * one kernel into the two full-format staging buffers of rs_msm_hostkey, and everything downstream reads those.  A
 * host-resident seeded key lands in two compact buffers beside them first: staging memory is 1.5 times rs_msm_hostkey's. */
int rs_msm_seeded(rs_ctx *ctx, const uint64_t *const *crs, const uint64_t *h_pub_seeds, int crs_on_host, int n_crs, size_t crs_len,
                  size_t crs_window, const rs_msm_vec *vecs, int n_vecs, int n_groups, uint64_t *d_out, size_t *h_used,
                  rs_stream stream);

/* rs_groth16_pk with compact vectors and their public seeds.  ZERO-INITIALISE the struct. */
typedef struct rs_groth16_pk_seeded {
  const uint64_t *s_pows, *delta_ts; /* [m+1] compact; host pointers when host_key */
  const uint64_t *delta_mid;         /* [n_aux] compact */
  uint64_t pub_seeds[3];             /* of s_pows, delta_ts, delta_mid */
  const uint64_t *d_alpha, *d_beta;  /* full elements on the device */
  size_t window;                     /* as in rs_groth16_pk */
  int host_key;
} rs_groth16_pk_seeded;
/* rs_groth16_prove_kinds on a seeded key; h_assignment_kinds may be NULL. */
int rs_groth16_prove_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, const uint64_t *d_assignment,
                            const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, rs_stream stream);

typedef struct rs_rinocchio_pk_seeded {
  const uint64_t *s_pows, *alpha_s_pows; /* [m+1] compact; host pointers when host_key */
  const uint64_t *beta_prods;            /* [n_aux] compact */
  uint64_t pub_seeds[3];                 /* of s_pows, alpha_s_pows, beta_prods */
  const uint64_t *d_beta_rv_ts, *d_beta_rw_ts, *d_beta_ry_ts; /* full elements on the device */
  size_t window;
  int host_key;
} rs_rinocchio_pk_seeded;
/* rs_rinocchio_prove_kinds on a seeded key; h_assignment_kinds may be NULL. */
int rs_rinocchio_prove_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, const uint64_t *d_assignment,
                              const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                              uint64_t *d_proof, int *h_empty, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
