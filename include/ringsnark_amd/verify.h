/* ringsnark_amd/verify.h -- C ABI of the two verifiers of librs_hip.so, present when rs_version() >= 103
 * (versions: 100 first ABI; 101 rs_msm_vec::slot_const, rs_enc_noise_budget, RS_ERR_NOISE; 102 r1cs_check.h; 103 this header).
 * Conventions as in ringsnark_amd.h, which this header includes: d_* device pointers, h_* host pointers, status codes,
 * rs_last_error.  Declared beside ringsnark_amd.h for the reason given in r1cs_check.h.
 *
 * groth16::verifier (zk_proof_systems/groth16/groth16.tcc:117-170) and rinocchio::verifier
 * (zk_proof_systems/rinocchio/rinocchio.tcc:192-295).  Both start with r1cs_to_qrp_instance_map_with_evaluation(cs, vk.s)
 * (groth16.tcc:127-128, rinocchio.tcc:219-221) and then evaluate the constraints on `primary || zeros`, interpolate three
 * length-m polynomials and run Horner at s (groth16.tcc:131-154, rinocchio.tcc:230-254).  Interpolation and evaluation are
 * linear and the ring is commutative, so that value is exactly
 *     v_io(s) = sum_{k = 0..n_inputs} x_k * A_k(s),  x_0 = 1          (likewise w_io with B_k, y_io with C_k)
 * with A_k(s) the entries of the instance map: a verifier needs Z(s) and the n_inputs + 1 PUBLIC columns of each matrix,
 * not the [n_vars+1][L][N] vectors of rs_instance_map_eval.  rs_io_eval_at computes exactly those, a verification key keeps
 * them, and one verification is a decode plus one small kernel.  All arithmetic is exact: every residue equals the
 * reference's (DESIGN.md "Verifier"). */
#ifndef RINGSNARK_AMD_VERIFY_H
#define RINGSNARK_AMD_VERIFY_H
#include "../ringsnark_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A_k(s), B_k(s), C_k(s) for k = 0..n_inputs (k = 0: the constant one) and Z(s) = prod_{j<m} (s - j).
 * d_s [L][N]; d_Aio, d_Bio, d_Cio [n_inputs+1][L][N]; d_Zt [L][N] (any output may be NULL).
 * Bit-identical to rows 0..n_inputs of rs_instance_map_eval's At/Bt/Ct and to its Zt.
 * Division free (u_j(s) = c_j * prod_{i != j} (s - i), c_j slot-constant), so s may coincide with a node in some slots;
 * RS_ERR_NOT_INVERTIBLE ("t cannot be one of the values in the domain") only when s is a domain element in every slot of
 * every limb (util/evaluation_domain.tcc:24-26).  Workspace: 2 * ceil(m / 64) ring elements and L * m words of constants
 * -- nothing proportional to m * L * N, no transposed system.  Synchronises. */
int rs_io_eval_at(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *d_Aio, uint64_t *d_Bio, uint64_t *d_Cio,
                  uint64_t *d_Zt, rs_stream stream);

/* groth16.hpp:50-86 verification_key: s, alpha, beta, gamma, delta [L][N] each, sk_enc [K][N_enc] in NTT form (as
 * rs_enc_decode takes it).  Runs rs_io_eval_at once and keeps device copies of the public columns, Z(s), the trapdoor
 * elements and the secret key; the constraint system is not referenced after the call.
 * gamma must be invertible -- the reference divides by it (groth16.tcc:162) -- else RS_ERR_NOT_INVERTIBLE ("element is not
 * invertible in ring").  Since gamma * (f / gamma) = f exactly for an invertible gamma, the verifier itself uses
 * f = beta * v_io + alpha * w_io + y_io directly and never divides.
 * rs_*_vk_destroy overwrites the key's device memory with zeros before freeing it. */
typedef struct rs_groth16_vk rs_groth16_vk;
int rs_groth16_vk_create(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                         const uint64_t *d_gamma, const uint64_t *d_delta, const uint64_t *d_sk, rs_groth16_vk **out);
void rs_groth16_vk_destroy(rs_groth16_vk *vk);
/* rinocchio.hpp:60-97 verification_key: s, alpha, beta, r_v, r_w, r_y, sk_enc. */
typedef struct rs_rinocchio_vk rs_rinocchio_vk;
int rs_rinocchio_vk_create(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                           const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                           rs_rinocchio_vk **out);
void rs_rinocchio_vk_destroy(rs_rinocchio_vk *vk);

/* What a verification found.  Every field is a function of the inputs only (no dependence on launch order).
 * Checks and the two sides compared (lhs, rhs):
 *   groth16    0: A * B                  ==  alpha * beta + f + delta * C                   (groth16.tcc:164-169)
 *   rinocchio  0: V'  == alpha * V    1: W' == alpha * W    2: Y' == alpha * Y    3: H' == alpha * H     (rinocchio.tcc:262-282)
 *              4: beta * (r_v V + r_w W + r_y Y)  ==  L_beta   -- skipped when the last proof element is EMPTY (:199-206, 283-288)
 *              5: (V + v_io)(W + w_io) - (Y + y_io)  ==  H * Z(s)                           (rinocchio.tcc:256-259, 289-293)
 *   with (V, V', W, W', Y, Y', H, H', L_beta) the decodings of proof elements 0..8. */
typedef struct rs_verify_report {
  uint32_t accepted;      /* the reference's return value */
  uint32_t failed;        /* bit c set: check c fails in some slot */
  uint64_t n_bad[6];      /* ring-layout positions (limb*N + slot) at which check c fails */
  uint32_t first_check, first_limb, first_slot; /* lowest failing check, then lowest position in it; 0 if accepted */
  uint64_t lhs, rhs;      /* the two canonical residues compared there; 0 if accepted */
} rs_verify_report;
/* d_primary [n_inputs][L][N] (may be NULL when n_inputs == 0); d_proof: 3 ({A, B, C}) resp. 9 ({A, A', B, B', C, C', D, D', F},
 * as rs_rinocchio_prove writes them) encoding elements; h_empty[k] != 0: element k is EMPTY and counts as the zero ring
 * element (its payload is not read).  The other elements are decoded as rs_enc_decode does, noise guard on: a spent
 * budget returns RS_ERR_NOISE with the reference's message -- the reference's verifier throws there too
 * (seal_ring.tcc:446-454).  Returns RS_OK whether the proof is accepted or rejected: a rejection is an answer, not an
 * error.  A key is bound to the context it was created on (RS_ERR_INVALID otherwise) and is only read; calls on one
 * context serialise.  Synchronise. */
int rs_groth16_verify(rs_ctx *ctx, const rs_groth16_vk *vk, const uint64_t *d_primary, const uint64_t *d_proof,
                      const int *h_empty /* [3] or NULL */, rs_verify_report *h_report, rs_stream stream);
int rs_rinocchio_verify(rs_ctx *ctx, const rs_rinocchio_vk *vk, const uint64_t *d_primary, const uint64_t *d_proof,
                        const int *h_empty /* [9] or NULL */, rs_verify_report *h_report, rs_stream stream);
#ifdef __cplusplus
}
#endif
#endif
