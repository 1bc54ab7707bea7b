// packed.hip -- bit-packed seeded proving keys (include/ringsnark_amd/packed.h): the c0 rows of a seeded vector stored as
// little-endian bit streams of w = max_j bitlen(Q_j) bits a residue.  This file: the pack / unpack / expansion kernels and the
// entry points; the tile loop that calls the expansion kernel is in msm.hip (msm_run), the generators' tile loop in keygen.hip
// (encode_vector), the provers' bodies in prover.hip.  The kernels move integers only: both arithmetics are served.
#include <algorithm>

#include "../../include/ringsnark_amd/batch.h"
#include "../../include/ringsnark_amd/packed.h"
#include "rs_internal.hpp"

namespace rs {

// A row is cut as expand_seeded_tile_kernel cuts it: one workgroup per row, or per EXPAND_SPAN = 2048 coefficients of it.  A
// part of 2048 coefficients is 2048 w / 64 = 32 w words, so every part starts on a word boundary and a 16-byte boundary; a row
// of fewer than 2048 coefficients is one part of row_words words (a partial last word and up to one zero pad word).
constexpr int PACK_SEG_WORDS = 32 * 62;  // the longest part, at w = 62: 15.5 KiB
struct PackGeom {
  int w, parts, span, part_words;
  size_t row_words;
};

int pack_bits(const rs_ctx *ctx) {
  int w = 0;
  for (int j = 0; j < ctx->K; j++) w = std::max(w, 64 - __builtin_clzll(ctx->Q[j] | 1));
  RS_REQUIRE(w >= 2 && w <= 62, "data prime out of range");
  return w;
}
size_t packed_row_words(const rs_ctx *ctx) { return 2 * (((size_t)ctx->N_enc * pack_bits(ctx) + 127) / 128); }

static PackGeom pack_geom(const rs_ctx *ctx) {
  const int n = ctx->N_enc;
  PackGeom g;
  g.w = pack_bits(ctx);
  g.parts = std::max(1, n / EXPAND_SPAN);
  g.span = n / g.parts;
  RS_REQUIRE(n >= 2 && n % 2 == 0 && n % g.parts == 0 && (g.parts == 1 ? n <= EXPAND_SPAN : g.span == EXPAND_SPAN), "encoding degree out of range");
  g.row_words = packed_row_words(ctx);
  g.part_words = g.parts == 1 ? (int)g.row_words : 32 * g.w;
  RS_REQUIRE((size_t)g.part_words * g.parts == g.row_words && g.part_words <= PACK_SEG_WORDS, "encoding degree out of range");
  return g;
}

// residue p of the part whose words are seg[]: bits [p w, (p + 1) w).  The second word is read only when the residue
// straddles, and then sh > 0: no shift by 64.
__device__ __forceinline__ uint64_t packed_residue(const uint64_t *seg, int p, int w, uint64_t mask) {
  const unsigned bit = (unsigned)p * (unsigned)w, wi = bit >> 6, sh = bit & 63;
  uint64_t v = seg[wi] >> sh;
  if (sh + (unsigned)w > 64) v |= seg[wi + 1] << (64 - sh);
  return v & mask;
}
// the part's words global -> LDS in 16-byte loads, consecutive lanes on consecutive words
__device__ __forceinline__ void stage_part(uint64_t *seg, const uint64_t *src, int words) {
  const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(src);
  ulonglong2 *d = reinterpret_cast<ulonglong2 *>(seg);
  for (int k = (int)threadIdx.x; k < words / 2; k += EXPAND_THREADS) d[k] = s[k];
  __syncthreads();
}
// word k of a part from its residues res[0 .. span): residues floor(64 k / w) .. while they start below bit 64 k + 64; bits
// past the last residue stay zero (the padding of a short row)
__device__ __forceinline__ uint64_t packed_word(const uint64_t *res, int k, int w, int span, uint64_t mask) {
  const int b0 = k * 64;
  int p = b0 / w, off = p * w - b0;  // off in (-w, 0]
  uint64_t acc = 0;
  for (; off < 64 && p < span; off += w, p++) {
    const uint64_t v = res[p] & mask;
    acc |= off < 0 ? v >> (-off) : v << off;
  }
  return acc;
}

// c0: [rows][n] -> packed: [rows][row_words], rows = count L K.  bad: nullptr, or the count of input words >= 2^w (one
// atomic per thread that saw one; clean input issues none).
__global__ void __launch_bounds__(EXPAND_THREADS)
pack_c0_kernel(const uint64_t *__restrict__ c0, uint64_t *__restrict__ packed, unsigned long long *__restrict__ bad, int n, PackGeom g) {
  __shared__ __attribute__((aligned(16))) uint64_t res[EXPAND_SPAN];
  const size_t row = blockIdx.x / (unsigned)g.parts;
  const int part = (int)(blockIdx.x % (unsigned)g.parts);
  const uint64_t mask = (1ull << g.w) - 1;
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(c0 + row * (size_t)n + (size_t)part * g.span);
  unsigned n_bad = 0;
  for (int k = (int)threadIdx.x; k < g.span / 2; k += EXPAND_THREADS) {
    const ulonglong2 v = src[k];
    n_bad += (v.x > mask) + (v.y > mask);
    reinterpret_cast<ulonglong2 *>(res)[k] = v;
  }
  if (bad && n_bad) atomicAdd(bad, (unsigned long long)n_bad);
  __syncthreads();
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(packed + row * g.row_words + (size_t)part * g.part_words);
  for (int k = (int)threadIdx.x; k < g.part_words / 2; k += EXPAND_THREADS) {
    ulonglong2 o;
    o.x = packed_word(res, 2 * k, g.w, g.span, mask);
    o.y = packed_word(res, 2 * k + 1, g.w, g.span, mask);
    dst[k] = o;
  }
}

__global__ void __launch_bounds__(EXPAND_THREADS)
unpack_c0_kernel(const uint64_t *__restrict__ packed, uint64_t *__restrict__ c0, int n, PackGeom g) {
  __shared__ __attribute__((aligned(16))) uint64_t seg[PACK_SEG_WORDS];
  const size_t row = blockIdx.x / (unsigned)g.parts;
  const int part = (int)(blockIdx.x % (unsigned)g.parts);
  const uint64_t mask = (1ull << g.w) - 1;
  stage_part(seg, packed + row * g.row_words + (size_t)part * g.part_words, g.part_words);
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(c0 + row * (size_t)n + (size_t)part * g.span);
  for (int p = 2 * (int)threadIdx.x; p < g.span; p += 2 * EXPAND_THREADS) {
    ulonglong2 o;
    o.x = packed_residue(seg, p, g.w, mask);
    o.y = packed_residue(seg, p + 1, g.w, mask);
    dst[p >> 1] = o;
  }
}

// expand_seeded_tile_kernel with packed c0 rows: the same blocks, indices and streams; the part's words are staged in LDS,
// c0 is unpacked from there and c1 regenerated, both written in 16-byte stores.
// enc: [count][L][2][K][n].  packed: [.][L][K][row_words], element i read at index i (linear) or at its stored index.
__global__ void __launch_bounds__(EXPAND_THREADS)
expand_packed_tile_kernel(const uint64_t *__restrict__ packed, uint64_t *__restrict__ enc, uint64_t pub_seed, size_t first, size_t window,
                          int linear, int L, int K, int n, PackGeom g, ExpandPrimes pr) {
  __shared__ __attribute__((aligned(16))) uint64_t seg[PACK_SEG_WORDS];
  const size_t row = blockIdx.x / (unsigned)g.parts;
  const int part = (int)(blockIdx.x % (unsigned)g.parts);
  const int j = (int)(row % (size_t)K);
  const size_t el = row / (size_t)K;  // (element, limb)
  const int limb = (int)(el % (size_t)L);
  const size_t i = el / (size_t)L;
  const size_t stored = window ? (first + i) % window : first + i;
  const uint64_t seed = (pub_seed + stored) * 1315423911ull + (uint64_t)limb + 1;  // as keygen_encode_kernel's pseed
  const uint64_t Q = pr.Q[j], mu = pr.mu[j], mask = (1ull << g.w) - 1;
  const uint64_t draw0 = (uint64_t)n + (uint64_t)j * n + 1;  // draw of a_j[0]
  stage_part(seg, packed + (((linear ? i : stored) * L + limb) * K + j) * g.row_words + (size_t)part * g.part_words, g.part_words);
  uint64_t *d0 = enc + (el * 2 * K + j) * (size_t)n;
  ulonglong2 *dst0 = reinterpret_cast<ulonglong2 *>(d0), *dst1 = reinterpret_cast<ulonglong2 *>(d0 + (size_t)K * n);
  const int base = part * g.span;
  for (int p = 2 * (int)threadIdx.x; p < g.span; p += 2 * EXPAND_THREADS) {
    ulonglong2 c, a;
    c.x = packed_residue(seg, p, g.w, mask);
    c.y = packed_residue(seg, p + 1, g.w, mask);
    dst0[(base + p) >> 1] = c;
    a.x = barrett_mod(splitmix_at(seed, draw0 + (uint64_t)(base + p)), Q, mu);
    a.y = barrett_mod(splitmix_at(seed, draw0 + (uint64_t)(base + p) + 1), Q, mu);
    dst1[(base + p) >> 1] = a;
  }
}

static unsigned pack_blocks(const rs_ctx *ctx, const PackGeom &g, size_t count) {
  const size_t blocks = count * (size_t)ctx->L * ctx->K * g.parts;
  RS_REQUIRE(blocks < ((size_t)1 << 31), "too many elements for one launch");
  return (unsigned)blocks;
}

void pack_c0_run(rs_ctx *ctx, const uint64_t *c0, size_t count, uint64_t *packed, unsigned long long *d_bad, hipStream_t st) {
  if (count == 0) return;
  const PackGeom g = pack_geom(ctx);
  RS_REQUIRE(((uintptr_t)c0 | (uintptr_t)packed) % 16 == 0, "packed key vectors and their compact form must be 16-byte aligned");
  const unsigned blocks = pack_blocks(ctx, g, count);
  const double rows = (double)count * ctx->L * ctx->K;
  ProfScope p(ctx, st, "pack_c0_kernel", rows * 8.0 * ((double)ctx->N_enc + (double)g.row_words), 0.0);
  hipLaunchKernelGGL(pack_c0_kernel, dim3(blocks), dim3(EXPAND_THREADS), 0, st, c0, packed, d_bad, ctx->N_enc, g);
  RS_HIP(hipGetLastError());
}

static void unpack_c0_run(rs_ctx *ctx, const uint64_t *packed, size_t count, uint64_t *c0, hipStream_t st) {
  if (count == 0) return;
  const PackGeom g = pack_geom(ctx);
  RS_REQUIRE(((uintptr_t)c0 | (uintptr_t)packed) % 16 == 0, "packed key vectors and their compact form must be 16-byte aligned");
  const unsigned blocks = pack_blocks(ctx, g, count);
  const double rows = (double)count * ctx->L * ctx->K;
  ProfScope p(ctx, st, "unpack_c0_kernel", rows * 8.0 * ((double)ctx->N_enc + (double)g.row_words), 0.0);
  hipLaunchKernelGGL(unpack_c0_kernel, dim3(blocks), dim3(EXPAND_THREADS), 0, st, packed, c0, ctx->N_enc, g);
  RS_HIP(hipGetLastError());
}

void expand_packed_run(rs_ctx *ctx, const uint64_t *packed, bool linear, uint64_t pub_seed, size_t first, size_t window, size_t count,
                       uint64_t *dst, hipStream_t st) {
  if (count == 0) return;
  const PackGeom g = pack_geom(ctx);
  RS_REQUIRE(((uintptr_t)packed | (uintptr_t)dst) % 16 == 0, "packed key vectors and their expansion must be 16-byte aligned");
  const unsigned blocks = pack_blocks(ctx, g, count);
  const ExpandPrimes pr = expand_primes(ctx);
  const double rows = (double)count * ctx->L * ctx->K;
  // algorithmic bytes: the packed rows read, both components written; no FP64 work
  ProfScope p(ctx, st, "expand_packed_tile_kernel", rows * 8.0 * ((double)g.row_words + 2.0 * ctx->N_enc), 0.0);
  hipLaunchKernelGGL(expand_packed_tile_kernel, dim3(blocks), dim3(EXPAND_THREADS), 0, st, packed, dst, pub_seed, first, window,
                     linear ? 1 : 0, ctx->L, ctx->K, ctx->N_enc, g, pr);
  RS_HIP(hipGetLastError());
}

// A packed key in the full key's struct, as the provers' bodies take it beside pk->pub_seeds and the packed mark.  The
// vectors are checked here, before the witness map writes anything.
static void require_aligned(const void *a, const void *b, const void *c) {
  RS_REQUIRE(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0, "packed key vectors must be 16-byte aligned");
}
static rs_groth16_pk full_format(const rs_groth16_pk_seeded *pk) {
  RS_REQUIRE(pk != nullptr, "null argument");
  require_aligned(pk->s_pows, pk->delta_ts, pk->delta_mid);
  return {pk->s_pows, pk->delta_ts, pk->delta_mid, pk->d_alpha, pk->d_beta, pk->window, pk->host_key};
}
static rs_rinocchio_pk full_format(const rs_rinocchio_pk_seeded *pk) {
  RS_REQUIRE(pk != nullptr, "null argument");
  require_aligned(pk->s_pows, pk->alpha_s_pows, pk->beta_prods);
  return {pk->s_pows, pk->alpha_s_pows, pk->beta_prods, pk->d_beta_rv_ts, pk->d_beta_rw_ts, pk->d_beta_ry_ts, pk->window, pk->host_key};
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_enc_pack_bits(const rs_ctx *ctx) {
  RS_API_BEGIN
  RS_REQUIRE(ctx != nullptr, "null context");
  return pack_bits(ctx);
  }
  catch (const std::exception &e) {
    set_last_error(e.what());
    return 0;
  }
}

size_t rs_enc_packed_words(const rs_ctx *ctx) {
  RS_API_BEGIN
  RS_REQUIRE(ctx != nullptr, "null context");
  return packed_words(ctx);
  }
  catch (const std::exception &e) {
    set_last_error(e.what());
    return 0;
  }
}

int rs_enc_pack_c0(rs_ctx *ctx, const uint64_t *d_c0, size_t count, uint64_t *d_packed, size_t *h_bad, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(count == 0 || (d_c0 && d_packed), "null argument");
  hipStream_t st = S(stream);
  WsScope ws_scope(ctx, st);
  unsigned long long *d_bad = nullptr;
  if (h_bad && count) {
    d_bad = (unsigned long long *)ws_get(ctx, WS_SMALL, 256);
    RS_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), st));
  }
  pack_c0_run(ctx, d_c0, count, d_packed, d_bad, st);
  if (h_bad) {
    unsigned long long h = 0;
    if (d_bad) {
      RS_HIP(hipMemcpyAsync(&h, d_bad, sizeof(h), hipMemcpyDeviceToHost, st));
      RS_HIP(hipStreamSynchronize(st));
    }
    *h_bad = (size_t)h;
  }
  RS_API_END
}

int rs_enc_unpack_c0(rs_ctx *ctx, const uint64_t *d_packed, size_t count, uint64_t *d_c0, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(count == 0 || (d_c0 && d_packed), "null argument");
  WsScope ws_scope(ctx, S(stream));
  unpack_c0_run(ctx, d_packed, count, d_c0, S(stream));
  RS_API_END
}

int rs_enc_expand_packed(rs_ctx *ctx, const uint64_t *d_packed, uint64_t pub_seed, size_t first, size_t count, uint64_t *d_enc,
                         rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(count == 0 || (d_packed && d_enc), "null argument");
  WsScope ws_scope(ctx, S(stream));
  expand_packed_run(ctx, d_packed, true, pub_seed, first, 0, count, d_enc, S(stream));
  RS_API_END
}

int rs_groth16_keygen_packed(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                             const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const uint64_t h_pub_seeds[5],
                             const rs_groth16_seeded_key_out *out, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr && h_pub_seeds != nullptr, "null argument");
  require_aligned(out->s_pows, out->delta_ts, out->delta_mid);
  const uint64_t *trap[3] = {d_alpha, d_beta, d_delta};
  uint64_t *dst[5] = {out->s_pows, out->delta_ts, out->delta_mid, out->d_alpha, out->d_beta};
  keygen_run_scheme(0, ctx, cs, d_s, trap, d_sk, h_seeds, h_pub_seeds, dst, out->host_key != 0, out->tile, S(stream), true);
  RS_API_END
}

int rs_rinocchio_keygen_packed(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                               const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                               const uint64_t h_seeds[6], const uint64_t h_pub_seeds[6], const rs_rinocchio_seeded_key_out *out,
                               rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr && h_pub_seeds != nullptr, "null argument");
  require_aligned(out->s_pows, out->alpha_s_pows, out->beta_prods);
  const uint64_t *trap[5] = {d_alpha, d_beta, d_rv, d_rw, d_ry};
  uint64_t *dst[6] = {out->s_pows, out->alpha_s_pows, out->beta_prods, out->d_beta_rv_ts, out->d_beta_rw_ts, out->d_beta_ry_ts};
  keygen_run_scheme(1, ctx, cs, d_s, trap, d_sk, h_seeds, h_pub_seeds, dst, out->host_key != 0, out->tile, S(stream), true);
  RS_API_END
}

int rs_msm_packed(rs_ctx *ctx, const uint64_t *const *crs, const uint64_t *h_pub_seeds, int crs_on_host, int n_crs, size_t crs_len,
                  size_t crs_window, const rs_msm_vec *vecs, int n_vecs, int n_groups, uint64_t *d_out, size_t *h_used,
                  rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(crs && h_pub_seeds && vecs && d_out && n_vecs >= 1, "null argument");
  RS_REQUIRE(crs_on_host == 0 || crs_on_host == 1, "crs_on_host must be 0 or 1");
  RS_REQUIRE(n_crs >= 1 && n_crs <= 2, "n_crs must be 1 or 2");
  for (int c = 0; c < n_crs; c++) RS_REQUIRE(crs[c] && (uintptr_t)crs[c] % 16 == 0, "packed key vectors must be 16-byte aligned");
  WsScope ws_scope(ctx, S(stream));
  msm_run(ctx, MsmKey{crs, n_crs, crs_len, crs_window, crs_on_host != 0, h_pub_seeds, true}, vecs, n_vecs, n_groups, d_out, nullptr, h_used,
          S(stream));
  if (crs_on_host) RS_HIP(hipStreamSynchronize(S(stream)));  // the caller may release or rewrite the host key on return
  RS_API_END
}

int rs_groth16_prove_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, const uint64_t *d_assignment,
                            const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_groth16_pk full = full_format(pk);
  groth16_prove_members(ctx, cs, &full, pk->pub_seeds, 1, &d_assignment, h_assignment_kinds, d_proof, h_empty, false, S(stream), true);
  RS_API_END
}

int rs_rinocchio_prove_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, const uint64_t *d_assignment,
                              const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                              uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_rinocchio_pk full = full_format(pk);
  const uint64_t *d[3] = {d_d1, d_d2, d_d3};
  rinocchio_prove_members(ctx, cs, &full, pk->pub_seeds, 1, &d_assignment, h_assignment_kinds, d, d_proof, h_empty, false, S(stream), true);
  RS_API_END
}

int rs_groth16_prove_batch_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk_seeded *pk, int batch,
                                  const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, uint64_t *d_proofs,
                                  int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_groth16_pk full = full_format(pk);
  groth16_prove_members(ctx, cs, &full, pk->pub_seeds, batch, d_assignments, h_assignment_kinds, d_proofs, h_empty, true, S(stream), true);
  RS_API_END
}

int rs_rinocchio_prove_batch_packed(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk_seeded *pk, int batch,
                                    const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, const uint64_t *d_d123,
                                    uint64_t *d_proofs, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const rs_rinocchio_pk full = full_format(pk);
  const size_t rw = ctx->ring_words();
  const uint64_t *d[3] = {d_d123, d_d123 ? d_d123 + rw : nullptr, d_d123 ? d_d123 + 2 * rw : nullptr};
  rinocchio_prove_members(ctx, cs, &full, pk->pub_seeds, batch, d_assignments, h_assignment_kinds, d, d_proofs, h_empty, true, S(stream),
                          true);
  RS_API_END
}

}  // extern "C"
