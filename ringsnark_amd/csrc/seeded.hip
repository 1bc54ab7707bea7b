// seeded.hip -- seeded proving keys (include/ringsnark_amd/seeded.h): a key vector is stored as its c0 halves and one public
// seed, and c1 -- a counter-based stream (keygen.hip, keygen_encode_kernel: draw n + j n + p + 1 of the element's per-limb
// stream, % Q_j) -- is regenerated where the key is read.  This file: the expansion kernel and the entry points; the
// generators' template flag is in keygen.hip, the tile loop that calls the kernel in msm.hip (msm_run), the provers' bodies
// in prover.hip.
#include <algorithm>

#include "../../include/ringsnark_amd/batch.h"
#include "rs_internal.hpp"

namespace rs {

// One workgroup per (element, limb, prime) row, or per EXPAND_SPAN coefficients of it: Q_j and the stream seed are uniform
// in the workgroup.  c0 moves in 16-byte words; c1 is two draws per 16-byte store.
// enc: [count][L][2][K][n].  c0: [.][L][K][n], element i read at index i (linear) or at its stored index.
__global__ void __launch_bounds__(EXPAND_THREADS)
expand_seeded_tile_kernel(const uint64_t *__restrict__ c0, uint64_t *__restrict__ enc, uint64_t pub_seed, size_t first, size_t window,
                          int linear, int L, int K, int n, int parts, ExpandPrimes pr) {
  const size_t row = blockIdx.x / (unsigned)parts;
  const int part = (int)(blockIdx.x % (unsigned)parts);
  const int j = (int)(row % (size_t)K);
  const size_t el = row / (size_t)K;  // (element, limb)
  const int limb = (int)(el % (size_t)L);
  const size_t i = el / (size_t)L;
  const size_t stored = window ? (first + i) % window : first + i;
  const uint64_t seed = (pub_seed + stored) * 1315423911ull + (uint64_t)limb + 1;  // as keygen_encode_kernel's pseed
  const uint64_t Q = pr.Q[j], mu = pr.mu[j];
  const uint64_t draw0 = (uint64_t)n + (uint64_t)j * n + 1;  // draw of a_j[0]
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(c0 + (((linear ? i : stored) * L + limb) * K + j) * (size_t)n);
  uint64_t *d0 = enc + (el * 2 * K + j) * (size_t)n;
  ulonglong2 *dst0 = reinterpret_cast<ulonglong2 *>(d0), *dst1 = reinterpret_cast<ulonglong2 *>(d0 + (size_t)K * n);
  const int span = n / parts, end = (part + 1) * span;
  for (int p = part * span + 2 * (int)threadIdx.x; p < end; p += 2 * EXPAND_THREADS) {
    dst0[p >> 1] = src[p >> 1];
    ulonglong2 a;
    a.x = barrett_mod(splitmix_at(seed, draw0 + (uint64_t)p), Q, mu);
    a.y = barrett_mod(splitmix_at(seed, draw0 + (uint64_t)p + 1), Q, mu);
    dst1[p >> 1] = a;
  }
}

void expand_seeded_run(rs_ctx *ctx, const uint64_t *c0, bool linear, uint64_t pub_seed, size_t first, size_t window, size_t count,
                       uint64_t *dst, hipStream_t st) {
  if (count == 0) return;
  const int n = ctx->N_enc, parts = std::max(1, n / EXPAND_SPAN);
  RS_REQUIRE(n % 2 == 0 && n % parts == 0 && (n / parts) % 2 == 0, "encoding degree out of range");
  RS_REQUIRE(((uintptr_t)c0 | (uintptr_t)dst) % 16 == 0, "seeded key vectors and their expansion must be 16-byte aligned");
  const size_t blocks = count * (size_t)ctx->L * ctx->K * parts;
  RS_REQUIRE(blocks < ((size_t)1 << 31), "too many elements for one launch");
  const ExpandPrimes pr = expand_primes(ctx);
  const double words = (double)count * (double)ctx->enc_words();
  // algorithmic bytes: c0 read, both components written; no FP64 work
  ProfScope p(ctx, st, "expand_seeded_tile_kernel", words * 8.0 * 1.5, 0.0);
  hipLaunchKernelGGL(expand_seeded_tile_kernel, dim3((unsigned)blocks), dim3(EXPAND_THREADS), 0, st, c0, dst, pub_seed, first, window,
                     linear ? 1 : 0, ctx->L, ctx->K, n, parts, pr);
  RS_HIP(hipGetLastError());
}

// A seeded key in the full key's struct, as the provers' bodies take it beside pk->pub_seeds: the same vectors, compact
static rs_groth16_pk full_format(const rs_groth16_pk_seeded *pk) {
  RS_REQUIRE(pk != nullptr, "null argument");
  return {pk->s_pows, pk->delta_ts, pk->delta_mid, pk->d_alpha, pk->d_beta, pk->window, pk->host_key};
}
static rs_rinocchio_pk full_format(const rs_rinocchio_pk_seeded *pk) {
  RS_REQUIRE(pk != nullptr, "null argument");
  return {pk->s_pows, pk->alpha_s_pows, pk->beta_prods, pk->d_beta_rv_ts, pk->d_beta_rw_ts, pk->d_beta_ry_ts, pk->window, pk->host_key};
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_enc_expand_seeded(rs_ctx *ctx, const uint64_t *d_c0, uint64_t pub_seed, size_t first, size_t count, uint64_t *d_enc,
                         rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(count == 0 || (d_c0 && d_enc), "null argument");
  WsScope ws_scope(ctx, S(stream));  // ProfScope records into the context
  expand_seeded_run(ctx, d_c0, true, pub_seed, first, 0, count, d_enc, S(stream));
  RS_API_END
}

int rs_groth16_keygen_seeded(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                             const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const uint64_t h_pub_seeds[5],
                             const rs_groth16_seeded_key_out *out, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr && h_pub_seeds != nullptr, "null argument");
  const uint64_t *trap[3] = {d_alpha, d_beta, d_delta};
  uint64_t *dst[5] = {out->s_pows, out->delta_ts, out->delta_mid, out->d_alpha, out->d_beta};
  keygen_run_scheme(0, ctx, cs, d_s, trap, d_sk, h_seeds, h_pub_seeds, dst, out->host_key != 0, out->tile, S(stream));
  RS_API_END
}

int rs_rinocchio_keygen_seeded(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                               const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                               const uint64_t h_seeds[6], const uint64_t h_pub_seeds[6], const rs_rinocchio_seeded_key_out *out,
                               rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr && h_pub_seeds != nullptr, "null argument");
  const uint64_t *trap[5] = {d_alpha, d_beta, d_rv, d_rw, d_ry};
  uint64_t *dst[6] = {out->s_pows, out->alpha_s_pows, out->beta_prods, out->d_beta_rv_ts, out->d_beta_rw_ts, out->d_beta_ry_ts};
  keygen_run_scheme(1, ctx, cs, d_s, trap, d_sk, h_seeds, h_pub_seeds, dst, out->host_key != 0, out->tile, S(stream));
  RS_API_END
}

int rs_msm_seeded(rs_ctx *ctx, const uint64_t *const *crs, const uint64_t *h_pub_seeds, int crs_on_host, int n_crs, size_t crs_len,
                  size_t crs_window, const rs_msm_vec *vecs, int n_vecs, int n_groups, uint64_t *d_out, size_t *h_used,
                  rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(crs && h_pub_seeds && vecs && d_out && n_vecs >= 1, "null argument");
  RS_REQUIRE(crs_on_host == 0 || crs_on_host == 1, "crs_on_host must be 0 or 1");
  WsScope ws_scope(ctx, S(stream));
  msm_run(ctx, MsmKey{crs, n_crs, crs_len, crs_window, crs_on_host != 0, h_pub_seeds}, vecs, n_vecs, n_groups, d_out, nullptr, h_used,
          S(stream));
  if (crs_on_host) RS_HIP(hipStreamSynchronize(S(stream)));  // the caller may release or rewrite the host key on return
  RS_API_END
}

int rs_groth16_prove_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, const uint64_t *d_assignment,
                            const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_groth16_pk full = full_format(pk);
  groth16_prove_members(ctx, cs, &full, pk->pub_seeds, 1, &d_assignment, h_assignment_kinds, d_proof, h_empty, false, S(stream));
  RS_API_END
}

int rs_rinocchio_prove_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, const uint64_t *d_assignment,
                              const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                              uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_rinocchio_pk full = full_format(pk);
  const uint64_t *d[3] = {d_d1, d_d2, d_d3};
  rinocchio_prove_members(ctx, cs, &full, pk->pub_seeds, 1, &d_assignment, h_assignment_kinds, d, d_proof, h_empty, false, S(stream));
  RS_API_END
}

int rs_groth16_prove_batch_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, int batch,
                                  const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, uint64_t *d_proofs,
                                  int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_groth16_pk full = full_format(pk);
  groth16_prove_members(ctx, cs, &full, pk->pub_seeds, batch, d_assignments, h_assignment_kinds, d_proofs, h_empty, true, S(stream));
  RS_API_END
}

int rs_rinocchio_prove_batch_seeded(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, int batch,
                                    const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, const uint64_t *d_d123,
                                    uint64_t *d_proofs, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_rinocchio_pk full = full_format(pk);
  const size_t rw = ctx->ring_words();
  const uint64_t *d[3] = {d_d123, d_d123 ? d_d123 + rw : nullptr, d_d123 ? d_d123 + 2 * rw : nullptr};
  rinocchio_prove_members(ctx, cs, &full, pk->pub_seeds, batch, d_assignments, h_assignment_kinds, d, d_proofs, h_empty, true, S(stream));
  RS_API_END
}

}  // extern "C"
