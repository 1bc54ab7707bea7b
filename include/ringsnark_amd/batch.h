/* ringsnark_amd/batch.h -- C ABI of BATCHED proving of librs_hip.so, present when rs_version() >= 106
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 verify.h;
 * 104 keygen.h; 105 seeded.h; 106 this header, and rs_msm / rs_msm_hostkey / rs_msm_seeded accept up to
 * 4 RS_MAX_BATCH + 1 groups).  Conventions as in ringsnark_amd.h and seeded.h, which this header includes.  Declared
 * beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * A proving key does not depend on the assignment, and at the sizes where it lives in host memory (rs_groth16_pk::host_key,
 * seeded.h) reading it is most of a proof.  These calls prove `batch` assignments of ONE constraint system against ONE key
 * in one pass over every key vector: a tile of key elements is copied from the host (and, for a seeded key, expanded) once,
 * and multiplied into the plaintext rows of every member while it is on the device.  The witness map runs once per member.
 *
 * Proof b and h_empty[b] are WORD FOR WORD what the single-assignment call (rs_groth16_prove_kinds, rs_rinocchio_prove_kinds,
 * rs_groth16_prove_seeded, rs_rinocchio_prove_seeded) returns for assignment b on the same key -- full, windowed,
 * host-resident, seeded or both.  Every sum is exact modulo Q_j, so the order in which terms and groups are taken cannot
 * change a word.  batch == 1 is legal.  batch < 1 or batch > RS_MAX_BATCH: RS_ERR_INVALID, before anything is written.
 *
 * MEMORY.  The witness vectors of every member are held at once: batch * (5m+1) ring elements for ringGroth16 and
 * batch * (4m+1) for Rinocchio, in the context's workspace -- at the 2^16-constraint headline that is TENS OF GiB PER
 * MEMBER.  rs_prove_batch_bytes tells what a call will hold, so that a caller can choose `batch`.
 * rs_last_timings reports the phases of the whole batch (witness_ms: all the witness maps). */
#ifndef RINGSNARK_AMD_BATCH_H
#define RINGSNARK_AMD_BATCH_H
#include "seeded.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RS_MAX_BATCH 8

/* d_assignments: HOST array of `batch` device pointers, each [n_vars][L][N] (primary then auxiliary wires).
 * h_assignment_kinds: [batch][n_vars] wire kinds (rs_groth16_prove_kinds), or NULL.
 * d_proofs: [batch][3] encoding elements (A, B, C of member b at 3 b).  h_empty: [batch][3], or NULL. */
int rs_groth16_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, int batch, const uint64_t *const *d_assignments,
                           const uint8_t *h_assignment_kinds, uint64_t *d_proofs, int *h_empty, rs_stream stream);
/* d_d123: [batch][3][L][N], the zero-knowledge ring elements d1, d2, d3 of every member, or NULL = non-ZK for all.
 * d_proofs: [batch][9] encoding elements in the order of rs_rinocchio_prove.  h_empty: [batch][9], or NULL.
 * The two products of coefficients_for_Z, which do not depend on the assignment, are computed once per batch. */
int rs_rinocchio_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, int batch, const uint64_t *const *d_assignments,
                             const uint8_t *h_assignment_kinds, const uint64_t *d_d123, uint64_t *d_proofs, int *h_empty,
                             rs_stream stream);
/* The same on a seeded key (seeded.h): every tile of the key is expanded once per batch. */
int rs_groth16_prove_batch_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, int batch,
                                  const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, uint64_t *d_proofs,
                                  int *h_empty, rs_stream stream);
int rs_rinocchio_prove_batch_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, int batch,
                                    const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, const uint64_t *d_d123,
                                    uint64_t *d_proofs, int *h_empty, rs_stream stream);

/* Bytes of context workspace that a batched proof of `batch` members holds (scheme: 0 ringGroth16, 1 Rinocchio), with the
 * tuning knobs as they are now and a device-resident full key without window: the witness vectors of every member, the
 * plaintext rows of the largest term tile, the partial accumulator sets, the inner products before they are copied into the
 * proofs, and the used-term words.  A host-resident or seeded key adds its staging buffers (2 n_crs msm_host_tile elements,
 * 1.5 times that for a host-resident seeded key), which do not depend on `batch`; the witness map's own workspace is that of
 * ONE proof.  Affine in `batch` as long as a term tile holds the longest vector (tuning knob msm_c_mib). */
int rs_prove_batch_bytes(rs_ctx *ctx, const rs_r1cs *cs, int scheme, int batch, size_t *h_bytes);
#ifdef __cplusplus
}
#endif
#endif
