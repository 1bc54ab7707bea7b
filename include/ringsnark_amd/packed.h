/* ringsnark_amd/packed.h -- C ABI of BIT-PACKED seeded proving keys of librs_hip.so, present when rs_version() >= 111
 * (versions: see seeded.h; 111 this header).  Conventions as in ringsnark_amd.h, keygen.h and seeded.h, which this header
 * includes.  Declared beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * Every residue of a key is a canonical value below a data prime Q_j and is stored in a 64-bit word; with 43/44-bit primes
 * 20 of every 64 bits are zero.  A packed vector ("RSPK") is a seeded vector (seeded.h: c0 only, c1 from the public seed)
 * whose c0 rows are bit streams:
 *     w         = max_j bitlen(Q_j) over the context's K data primes (2 <= w <= 62): ONE width per context;
 *     row       : the N_enc residues of one (element, limb, prime) row as a little-endian bit stream -- residue p occupies
 *                 bits [p w, (p + 1) w), bit b lives in word b >> 6 at position b & 63;
 *     row_words = 2 ceil(N_enc w / 128): every row is 16-byte aligned; padding bits are zero (deterministic bytes);
 *     vector    : [count][L][K][row_words], the rows in the order of the compact layout [count][L][K][N_enc].
 * Seeds, stream derivation, the window / stored-index rule and the disjointness checks are those of seeded.h.  Packing is
 * lossless and public: nothing in the security notes of seeded.h changes.  Single elements of a key (alpha, beta, beta_r*_ts)
 * stay full-format.
 *
 * Every pointer to a packed, compact or full vector must be 16-byte aligned; an unaligned or null pointer, or intersecting
 * seed ranges, give RS_ERR_INVALID before anything is written. */
#ifndef RINGSNARK_AMD_PACKED_H
#define RINGSNARK_AMD_PACKED_H
#include "seeded.h"
#ifdef __cplusplus
extern "C" {
#endif

/* w of the context, and the words of one packed element, L K row_words. */
int rs_enc_pack_bits(const rs_ctx *ctx);
size_t rs_enc_packed_words(const rs_ctx *ctx);

/* compact [count][L][K][N_enc] -> packed [count][L][K][row_words].  The low w bits of every word are stored.  A word >= 2^w
 * is bad input and is an answer, not an error (as in bits.h): the call returns RS_OK and *h_bad, when h_bad is not NULL, is
 * the number of such words (the call then synchronises; otherwise it is asynchronous on `stream`). */
int rs_enc_pack_c0(rs_ctx *ctx, const uint64_t *d_c0, size_t count, uint64_t *d_packed, size_t *h_bad, rs_stream stream);
/* packed -> compact.  Asynchronous on `stream`. */
int rs_enc_unpack_c0(rs_ctx *ctx, const uint64_t *d_packed, size_t count, uint64_t *d_c0, rs_stream stream);
/* rs_enc_expand_seeded on packed elements: d_enc[i] (full format) for i < count from d_packed[i], c0 unpacked, c1 regenerated
 * from the stream of stored index first + i. */
int rs_enc_expand_packed(rs_ctx *ctx, const uint64_t *d_packed, uint64_t pub_seed, size_t first, size_t count, uint64_t *d_enc,
                         rs_stream stream);

/* The generators of seeded.h with the three vectors written PACKED ([.][L][K][row_words]), on the device or in host memory
 * (host_key, tile).  Every tile of at most `tile` elements (0: 64) is encoded compact into a staging buffer and packed from
 * there -- a device-resident key straight into its place, so it never exists unpacked.  The bytes are those of
 * rs_enc_pack_c0 applied to the vectors of the _seeded generator with the same arguments. */
int rs_groth16_keygen_packed(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                             const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const uint64_t h_pub_seeds[5],
                             const rs_groth16_seeded_key_out *out, rs_stream stream);
int rs_rinocchio_keygen_packed(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                               const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                               const uint64_t h_seeds[6], const uint64_t h_pub_seeds[6], const rs_rinocchio_seeded_key_out *out,
                               rs_stream stream);

/* rs_msm_seeded over PACKED key vectors: a stored element is rs_enc_packed_words words; a tile is expanded by one kernel
 * (c0 unpacked, c1 regenerated) into the staging buffers of rs_msm_seeded, and everything downstream reads those. */
int rs_msm_packed(rs_ctx *ctx, const uint64_t *const *crs, const uint64_t *h_pub_seeds, int crs_on_host, int n_crs, size_t crs_len,
                  size_t crs_window, const rs_msm_vec *vecs, int n_vecs, int n_groups, uint64_t *d_out, size_t *h_used,
                  rs_stream stream);

/* The provers of seeded.h and batch.h on a packed key.  The structs are those of seeded.h: the entry point, not the struct,
 * says that the three vectors are packed. */
int rs_groth16_prove_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, const uint64_t *d_assignment,
                            const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, rs_stream stream);
int rs_rinocchio_prove_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, const uint64_t *d_assignment,
                              const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                              uint64_t *d_proof, int *h_empty, rs_stream stream);
int rs_groth16_prove_batch_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, int batch,
                                  const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, uint64_t *d_proofs,
                                  int *h_empty, rs_stream stream);
int rs_rinocchio_prove_batch_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, int batch,
                                    const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, const uint64_t *d_d123,
                                    uint64_t *d_proofs, int *h_empty, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
