// prover.hip -- groth16::prover (row a15) and rinocchio::prover (row a16) on the device, plus the
// synthetic-workload generators used by the benchmark harness.
#include <algorithm>
#include <cstring>

#include "../../include/ringsnark_amd/batch.h"
#include "rs_internal.hpp"

namespace rs {
__global__ void __launch_bounds__(256) fill_ones_kernel(uint64_t *p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1;
}
static void fill_ones(rs_ctx *, uint64_t *p, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(fill_ones_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n);
}

struct PhaseTimer {
  rs_ctx *ctx;
  hipStream_t st;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  explicit PhaseTimer(rs_ctx *c, hipStream_t s) : ctx(c), st(s) {
    if (!ctx->profiling) return;
    for (auto &e : ev) RS_HIP(hipEventCreate(&e));
  }
  void mark(int k) {
    if (ctx->profiling) RS_HIP(hipEventRecord(ev[k], st));
  }
  void finish() {
    if (!ctx->profiling) return;
    RS_HIP(hipEventSynchronize(ev[2]));
    float w = 0, msm = 0;
    RS_HIP(hipEventElapsedTime(&w, ev[0], ev[1]));
    RS_HIP(hipEventElapsedTime(&msm, ev[1], ev[2]));
    ctx->timings.evaluate_ms = 0;
    ctx->timings.witness_ms = w;
    ctx->timings.msm_ms = msm;
    ctx->timings.total_ms = w + msm;
    for (auto &e : ev) (void)hipEventDestroy(e);
  }
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ void __launch_bounds__(256)
fill_uniform_kernel(uint64_t *__restrict__ dst, size_t words, size_t inner, int nmod, const uint64_t *__restrict__ mods,
                    uint64_t seed) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const uint64_t p = mods[(i / inner) % (size_t)nmod];
    dst[i] = mix64(mix64(seed) ^ (uint64_t)i) % p;
  }
}

// x_{i+2} = x_i * x_{i+1}; one thread per slot, values carried in registers.
template <class M>
__global__ void __launch_bounds__(256)
chain_kernel(uint64_t *__restrict__ asg, size_t m, int N, int L, const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t S = (size_t)L * N;
  const size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= S) return;
  const M mod = qmod[sl / (size_t)N];
  T a = center(from_res<T>(asg[sl]), mod), b = center(from_res<T>(asg[S + sl]), mod);
  for (size_t i = 0; i < m; i++) {
    const T c = reduce(mulmod_dd(a, b, mod), mod);
    asg[(i + 2) * S + sl] = to_res(canon(c, mod));
    a = b;
    b = c;
  }
}

// groth16::prover (groth16.tcc:70-115).  pub: nullptr, or the public seeds of s_pows, delta_ts, delta_mid of a seeded key.
void groth16_prove_run(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, const uint64_t *pub, const uint64_t *d_assignment,
                       const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, hipStream_t st) {
  RS_REQUIRE(ctx && cs && pk && d_assignment && d_proof, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_delta_ts && pk->d_alpha && pk->d_beta, "incomplete proving key");
  WsScope ws_scope(ctx, st);
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  RS_REQUIRE(n_aux == 0 || pk->d_delta_mid, "delta_mid missing");
  const bool host_key = pk->host_key != 0;
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  // witness map (groth16.tcc:82-84: d1 = d2 = d3 = 0); C_io / C_mid are not consumed by the prover
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (5 * m + 1) * rw * sizeof(uint64_t));
  uint64_t *A_io = wbuf, *A_mid = wbuf + m * rw, *B_io = wbuf + 2 * m * rw, *B_mid = wbuf + 3 * m * rw, *H = wbuf + 4 * m * rw;
  // The io vectors are linear forms of the primary inputs (witness.hip): when the inner product can take them in that
  // form (MsmLin) they are neither written by the witness map nor read and transformed by the inner product.
  const size_t nk = cs->n_inputs + 1;  // [1, x_1 .. x_n_inputs]; their encodings are staged in the (then unused) io rows
  const bool lin = g_tune.prover_lin_io && msm_supports_lin(ctx) && witness_io_shortcut(cs) &&
                   nk * std::max<size_t>(rw, (size_t)ctx->L * ctx->N_enc) <= m * rw;
  uint64_t *outs[7] = {lin ? nullptr : A_io, lin ? nullptr : B_io, nullptr, A_mid, B_mid, nullptr, H};
  witness_run(ctx, cs, d_assignment, nullptr, nullptr, nullptr, outs, nullptr, st);
  pt.mark(1);
  // A = <s_pows, A_io> + <s_pows, A_mid> + alpha ; B likewise with beta   (groth16.tcc:89-103)
  {
    const uint64_t *crs[1] = {pk->d_s_pows};
    const uint64_t *add[2] = {pk->d_alpha, pk->d_beta};
    if (lin) {
      // plaintexts of [1, x_1 .. x_n_inputs]: (n_inputs + 1) batch encodings, staged in the (unused) A_io rows
      uint64_t *rings = A_io, *P = B_io;  // [nk][L][N] and [nk][L][N_enc] words
      fill_ones(ctx, rings, rw, st);
      if (cs->n_inputs) RS_HIP(hipMemcpyAsync(rings + rw, d_assignment, cs->n_inputs * rw * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      batch_encode_run(ctx, rings, P, nk, st);
      MsmLin ln[2];
      for (int w = 0; w < 2; w++) {
        ln[w].k = cs->d_io_k[w];
        ln[w].col = cs->d_io_c[w];
        ln[w].count = cs->io_count[w];
        ln[w].Lcols = cs->d_io_cols;
        ln[w].Mlen = cs->io_M;
        ln[w].P = P;
        ln[w].T = m;
      }
      rs_msm_vec v[2] = {{A_mid, nullptr, m, 0}, {B_mid, nullptr, m, 1}};
      msm_run(ctx, crs, 1, m + 1, v, 2, 2, d_proof, add, nullptr, st, pk->window, ln, host_key, pub);
    } else {
      rs_msm_vec v[4] = {{A_io, nullptr, m, 0}, {A_mid, nullptr, m, 0}, {B_io, nullptr, m, 1}, {B_mid, nullptr, m, 1}};
      msm_run(ctx, crs, 1, m + 1, v, 4, 2, d_proof, add, nullptr, st, pk->window, nullptr, host_key, pub);
    }
  }
  // C = <delta_ts, H> (+ <delta_mid, aux>)                                 (groth16.tcc:105-112)
  size_t used_h = 1, used_aux = 0;
  uint64_t *C = d_proof + 2 * ew;
  if (n_aux) {
    const uint64_t *crs[1] = {pk->d_delta_mid};
    // the wires as the caller holds them: a Scalar-1 wire passes its key element through (seal_ring.tcc:525-527)
    rs_msm_vec v{d_assignment + cs->n_inputs * rw, h_assignment_kinds ? h_assignment_kinds + cs->n_inputs : nullptr, n_aux, 0};
    msm_run(ctx, crs, 1, n_aux, &v, 1, 1, C, nullptr, h_empty ? &used_aux : nullptr, st, pk->window, nullptr, host_key, pub ? pub + 2 : nullptr);
  }
  {
    const uint64_t *crs[1] = {pk->d_delta_ts};
    rs_msm_vec v{H, nullptr, m + 1, 0};
    const uint64_t *add[1] = {n_aux ? C : nullptr};
    msm_run(ctx, crs, 1, m + 1, &v, 1, 1, C, add, h_empty ? &used_h : nullptr, st, pk->window, nullptr, host_key, pub ? pub + 1 : nullptr);
  }
  pt.mark(2);
  pt.finish();
  if (host_key || h_assignment_kinds) RS_HIP(hipStreamSynchronize(st));  // the caller may release or rewrite the host key / the kinds on return
  if (h_empty) {
    h_empty[0] = h_empty[1] = 0;  // alpha / beta are always added
    h_empty[2] = (used_h == 0 && used_aux == 0) ? 1 : 0;
  }
}

// rinocchio::prover (rinocchio.tcc:75-190).  pub: nullptr, or the public seeds of s_pows, alpha_s_pows, beta_prods.
void rinocchio_prove_run(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, const uint64_t *pub, const uint64_t *d_assignment,
                         const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                         uint64_t *d_proof, int *h_empty, hipStream_t st) {
  RS_REQUIRE(ctx && cs && pk && d_assignment && d_proof, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_alpha_s_pows, "incomplete proving key");
  RS_REQUIRE((d_d1 && d_d2 && d_d3) || (!d_d1 && !d_d2 && !d_d3), "d1,d2,d3 must be all set or all null");
  WsScope ws_scope(ctx, st);
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  const bool zk = d_d1 != nullptr;  // rinocchio.tcc:81-90
  RS_REQUIRE(n_aux == 0 || pk->d_beta_prods, "beta_prods missing");
  RS_REQUIRE(!zk || n_aux == 0 || (pk->d_beta_rv_ts && pk->d_beta_rw_ts && pk->d_beta_ry_ts), "beta_r*_ts missing");
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (4 * m + 1) * rw * sizeof(uint64_t));
  uint64_t *A_mid = wbuf, *B_mid = wbuf + m * rw, *C_mid = wbuf + 2 * m * rw, *H = wbuf + 3 * m * rw;
  uint64_t *outs[7] = {nullptr, nullptr, nullptr, A_mid, B_mid, C_mid, H};
  witness_run(ctx, cs, d_assignment, d_d1, d_d2, d_d3, outs, nullptr, st);
  // coefficients_for_Z are slot constant: they go to the inner products as the compact [m+1][L] array of their values
  // (rs_msm_vec::slot_const) -- round 3 materialised m + 1 ring elements for them (a fifth of the prover's vectors).
  // A constant of the (context, m) plan: cached on the device, no host transpose and no synchronisation inside the proof.
  const uint64_t *dZ = witness_Z_rows(ctx, m);
  pt.mark(1);
  // the ten inner products of rinocchio.tcc:106-163 in one grouped pass over both CRS vectors
  uint64_t *mo = (uint64_t *)ws_get(ctx, WS_RINOCCHIO_OUT, 11 * ew * sizeof(uint64_t));  // [2][5] + tmp
  uint64_t *tmp = mo + 10 * ew;
  std::vector<uint8_t> zkinds(m + 1, RS_KIND_POLY);
  zkinds[m] = RS_KIND_ONE;  // leading coefficient of Z is the RingElem Scalar 1 (evaluation_domain.tcc:55-58)
  size_t used[5] = {0, 0, 0, 0, 0};
  {
    const uint64_t *crs[2] = {pk->d_s_pows, pk->d_alpha_s_pows};
    rs_msm_vec v[5] = {{A_mid, nullptr, m, 0}, {B_mid, nullptr, m, 1}, {C_mid, nullptr, m, 2}, {H, nullptr, m + 1, 3},
                       {dZ, zkinds.data(), m + 1, 4, 1}};
    msm_run(ctx, crs, 2, m + 1, v, 5, 5, mo, nullptr, used, st, pk->window, nullptr, pk->host_key != 0, pub);
  }
  auto slot = [&](int c, int g) { return mo + ((size_t)c * 5 + g) * ew; };
  int empty[9];
  for (int k = 0; k < 4; k++) {
    empty[2 * k] = empty[2 * k + 1] = used[k] == 0;
    RS_HIP(hipMemcpyAsync(d_proof + (size_t)(2 * k) * ew, slot(0, k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    RS_HIP(hipMemcpyAsync(d_proof + (size_t)(2 * k + 1) * ew, slot(1, k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  auto add_scaled = [&](uint64_t *dst, int *dst_empty, const uint64_t *enc, const uint64_t *d) {
    // dst += d * enc   (RingT * EncT then +=, rinocchio.tcc:168-173, 181-183)
    rs_msm_vec v{d, nullptr, 1, 0};
    const uint64_t *crs[1] = {enc};
    const uint64_t *add[1] = {*dst_empty ? nullptr : dst};
    msm_run(ctx, crs, 1, 1, &v, 1, 1, *dst_empty ? dst : tmp, add, nullptr, st, 0);
    if (!*dst_empty)
      RS_HIP(hipMemcpyAsync(dst, tmp, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    *dst_empty = 0;
  };
  if (zk) {  // rinocchio.tcc:167-174
    const uint64_t *ds[3] = {d_d1, d_d2, d_d3};
    for (int k = 0; k < 3; k++) {
      add_scaled(d_proof + (size_t)(2 * k) * ew, &empty[2 * k], slot(0, 4), ds[k]);
      add_scaled(d_proof + (size_t)(2 * k + 1) * ew, &empty[2 * k + 1], slot(1, 4), ds[k]);
    }
  }
  // F (rinocchio.tcc:176-185)
  empty[8] = 1;
  uint64_t *F = d_proof + 8 * ew;
  RS_HIP(hipMemsetAsync(F, 0, ew * sizeof(uint64_t), st));
  if (n_aux) {
    size_t used_f = 0;
    const uint64_t *crs[1] = {pk->d_beta_prods};
    rs_msm_vec v{d_assignment + cs->n_inputs * rw, h_assignment_kinds ? h_assignment_kinds + cs->n_inputs : nullptr, n_aux, 0};
    msm_run(ctx, crs, 1, n_aux, &v, 1, 1, F, nullptr, &used_f, st, pk->window, nullptr, pk->host_key != 0, pub ? pub + 2 : nullptr);
    empty[8] = used_f == 0;
    if (zk) {
      add_scaled(F, &empty[8], pk->d_beta_rv_ts, d_d1);
      add_scaled(F, &empty[8], pk->d_beta_rw_ts, d_d2);
      add_scaled(F, &empty[8], pk->d_beta_ry_ts, d_d3);
    }
  }
  pt.mark(2);
  pt.finish();
  RS_HIP(hipStreamSynchronize(st));  // zkinds is a host temporary referenced by async copies
  if (h_empty) memcpy(h_empty, empty, sizeof(empty));
}

// ---- batched proving (include/ringsnark_amd/batch.h): `batch` witness maps into slices of WS_PROVER_VECS, then ONE inner-
// product pass per key vector with the members' vectors as groups, so that a tile of the key is copied / expanded once.
static void require_batch(int batch, const uint64_t *const *d_assignments) {
  RS_REQUIRE(batch >= 1 && batch <= RS_MAX_BATCH, "batch must be in the range 1.." + std::to_string(RS_MAX_BATCH));
  RS_REQUIRE(d_assignments != nullptr, "null argument");
  for (int b = 0; b < batch; b++) RS_REQUIRE(d_assignments[b] != nullptr, "null assignment in the batch");
}

void groth16_prove_batch_run(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, const uint64_t *pub, int batch,
                             const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, uint64_t *d_proofs, int *h_empty,
                             hipStream_t st) {
  require_batch(batch, d_assignments);
  RS_REQUIRE(ctx && cs && pk && d_proofs, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_delta_ts && pk->d_alpha && pk->d_beta, "incomplete proving key");
  WsScope ws_scope(ctx, st);
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  RS_REQUIRE(n_aux == 0 || pk->d_delta_mid, "delta_mid missing");
  const bool host_key = pk->host_key != 0;
  const int B = batch;
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  const size_t per = (5 * m + 1) * rw;  // one member's vectors, laid out as in groth16_prove_run
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (size_t)B * per * sizeof(uint64_t));
  auto A_io = [&](int b) { return wbuf + (size_t)b * per; };
  auto A_mid = [&](int b) { return A_io(b) + m * rw; };
  auto B_io = [&](int b) { return A_io(b) + 2 * m * rw; };
  auto B_mid = [&](int b) { return A_io(b) + 3 * m * rw; };
  auto H = [&](int b) { return A_io(b) + 4 * m * rw; };
  const size_t nk = cs->n_inputs + 1;
  const bool lin = g_tune.prover_lin_io && msm_supports_lin(ctx) && witness_io_shortcut(cs) &&
                   nk * std::max<size_t>(rw, (size_t)ctx->L * ctx->N_enc) <= m * rw;
  for (int b = 0; b < B; b++) {  // the plan is shared; the maps run one after another
    uint64_t *outs[7] = {lin ? nullptr : A_io(b), lin ? nullptr : B_io(b), nullptr, A_mid(b), B_mid(b), nullptr, H(b)};
    witness_run(ctx, cs, d_assignments[b], nullptr, nullptr, nullptr, outs, nullptr, st);
  }
  pt.mark(1);
  // the inner products before they are copied into the proofs: [B][2] (A_b, B_b), [B] <delta_mid, aux_b>, [B] C_b
  uint64_t *ab = (uint64_t *)ws_get(ctx, WS_RINOCCHIO_OUT, (size_t)4 * B * ew * sizeof(uint64_t));
  uint64_t *cmid = ab + (size_t)2 * B * ew, *cfin = cmid + (size_t)B * ew;
  {  // pass 1 over s_pows: groups (A_b, B_b), alpha / beta added to every member's
    const uint64_t *crs[1] = {pk->d_s_pows};
    const uint64_t *add[2 * RS_MAX_BATCH];
    for (int b = 0; b < B; b++) {
      add[2 * b] = pk->d_alpha;
      add[2 * b + 1] = pk->d_beta;
    }
    if (lin) {
      MsmLin ln[2 * RS_MAX_BATCH];
      rs_msm_vec v[2 * RS_MAX_BATCH];
      for (int b = 0; b < B; b++) {
        // plaintexts of member b's [1, x_1 .. x_n_inputs], staged in ITS unused io rows
        uint64_t *rings = A_io(b), *P = B_io(b);
        fill_ones(ctx, rings, rw, st);
        if (cs->n_inputs) RS_HIP(hipMemcpyAsync(rings + rw, d_assignments[b], cs->n_inputs * rw * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        batch_encode_run(ctx, rings, P, nk, st);
        for (int w = 0; w < 2; w++) {
          MsmLin &l = ln[2 * b + w];
          l.k = cs->d_io_k[w];
          l.col = cs->d_io_c[w];
          l.count = cs->io_count[w];
          l.Lcols = cs->d_io_cols;
          l.Mlen = cs->io_M;
          l.P = P;
          l.T = m;
        }
        v[2 * b] = rs_msm_vec{A_mid(b), nullptr, m, 2 * b, 0};
        v[2 * b + 1] = rs_msm_vec{B_mid(b), nullptr, m, 2 * b + 1, 0};
      }
      msm_run(ctx, crs, 1, m + 1, v, 2 * B, 2 * B, ab, add, nullptr, st, pk->window, ln, host_key, pub, true);
    } else {
      rs_msm_vec v[4 * RS_MAX_BATCH];
      for (int b = 0; b < B; b++) {
        v[4 * b] = rs_msm_vec{A_io(b), nullptr, m, 2 * b, 0};
        v[4 * b + 1] = rs_msm_vec{A_mid(b), nullptr, m, 2 * b, 0};
        v[4 * b + 2] = rs_msm_vec{B_io(b), nullptr, m, 2 * b + 1, 0};
        v[4 * b + 3] = rs_msm_vec{B_mid(b), nullptr, m, 2 * b + 1, 0};
      }
      msm_run(ctx, crs, 1, m + 1, v, 4 * B, 2 * B, ab, add, nullptr, st, pk->window, nullptr, host_key, pub, true);
    }
  }
  size_t used_h[RS_MAX_BATCH], used_aux[RS_MAX_BATCH];
  for (int b = 0; b < B; b++) {
    used_h[b] = 1;
    used_aux[b] = 0;
  }
  if (n_aux) {  // pass 2 over delta_mid: the members' auxiliary wires as the caller holds them
    const uint64_t *crs[1] = {pk->d_delta_mid};
    rs_msm_vec v[RS_MAX_BATCH];
    for (int b = 0; b < B; b++)
      v[b] = rs_msm_vec{d_assignments[b] + cs->n_inputs * rw,
                        h_assignment_kinds ? h_assignment_kinds + (size_t)b * cs->n_vars + cs->n_inputs : nullptr, n_aux, b, 0};
    msm_run(ctx, crs, 1, n_aux, v, B, B, cmid, nullptr, h_empty ? used_aux : nullptr, st, pk->window, nullptr, host_key,
            pub ? pub + 2 : nullptr, true);
  }
  {  // pass 3 over delta_ts: H_b, with <delta_mid, aux_b> as addend
    const uint64_t *crs[1] = {pk->d_delta_ts};
    rs_msm_vec v[RS_MAX_BATCH];
    const uint64_t *add[RS_MAX_BATCH];
    for (int b = 0; b < B; b++) {
      v[b] = rs_msm_vec{H(b), nullptr, m + 1, b, 0};
      add[b] = n_aux ? cmid + (size_t)b * ew : nullptr;
    }
    msm_run(ctx, crs, 1, m + 1, v, B, B, cfin, add, h_empty ? used_h : nullptr, st, pk->window, nullptr, host_key, pub ? pub + 1 : nullptr,
            true);
  }
  for (int b = 0; b < B; b++) {
    uint64_t *proof = d_proofs + (size_t)3 * b * ew;
    RS_HIP(hipMemcpyAsync(proof, ab + (size_t)2 * b * ew, 2 * ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    RS_HIP(hipMemcpyAsync(proof + 2 * ew, cfin + (size_t)b * ew, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  pt.mark(2);
  pt.finish();
  if (host_key || h_assignment_kinds) RS_HIP(hipStreamSynchronize(st));  // the caller may release or rewrite the host key / the kinds on return
  if (h_empty)
    for (int b = 0; b < B; b++) {
      h_empty[3 * b] = h_empty[3 * b + 1] = 0;
      h_empty[3 * b + 2] = (used_h[b] == 0 && used_aux[b] == 0) ? 1 : 0;
    }
}

void rinocchio_prove_batch_run(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, const uint64_t *pub, int batch,
                               const uint64_t *const *d_assignments, const uint8_t *h_assignment_kinds, const uint64_t *d_d123,
                               uint64_t *d_proofs, int *h_empty, hipStream_t st) {
  require_batch(batch, d_assignments);
  RS_REQUIRE(ctx && cs && pk && d_proofs, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_alpha_s_pows, "incomplete proving key");
  WsScope ws_scope(ctx, st);
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  const bool zk = d_d123 != nullptr;
  RS_REQUIRE(n_aux == 0 || pk->d_beta_prods, "beta_prods missing");
  RS_REQUIRE(!zk || n_aux == 0 || (pk->d_beta_rv_ts && pk->d_beta_rw_ts && pk->d_beta_ry_ts), "beta_r*_ts missing");
  const int B = batch, NG = 4 * B + 1;  // groups: (a_b, b_b, c_b, h_b) per member, then Z, which every member shares
  auto dk = [&](int b, int k) { return zk ? d_d123 + ((size_t)3 * b + k) * rw : nullptr; };
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  const size_t per = (4 * m + 1) * rw;
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (size_t)B * per * sizeof(uint64_t));
  for (int b = 0; b < B; b++) {
    uint64_t *w = wbuf + (size_t)b * per;
    uint64_t *outs[7] = {nullptr, nullptr, nullptr, w, w + m * rw, w + 2 * m * rw, w + 3 * m * rw};
    witness_run(ctx, cs, d_assignments[b], dk(b, 0), dk(b, 1), dk(b, 2), outs, nullptr, st);
  }
  const uint64_t *dZ = witness_Z_rows(ctx, m);
  pt.mark(1);
  // [2][NG] inner products, [B] <beta_prods, aux_b>, one temporary
  uint64_t *mo = (uint64_t *)ws_get(ctx, WS_RINOCCHIO_OUT, (size_t)(2 * NG + B + 1) * ew * sizeof(uint64_t));
  uint64_t *fb = mo + (size_t)2 * NG * ew, *tmp = fb + (size_t)B * ew;
  std::vector<uint8_t> zkinds(m + 1, RS_KIND_POLY);
  zkinds[m] = RS_KIND_ONE;
  size_t used[4 * RS_MAX_BATCH + 1] = {0};
  {
    const uint64_t *crs[2] = {pk->d_s_pows, pk->d_alpha_s_pows};
    rs_msm_vec v[4 * RS_MAX_BATCH + 1];
    for (int b = 0; b < B; b++) {
      const uint64_t *w = wbuf + (size_t)b * per;
      v[4 * b] = rs_msm_vec{w, nullptr, m, 4 * b, 0};
      v[4 * b + 1] = rs_msm_vec{w + m * rw, nullptr, m, 4 * b + 1, 0};
      v[4 * b + 2] = rs_msm_vec{w + 2 * m * rw, nullptr, m, 4 * b + 2, 0};
      v[4 * b + 3] = rs_msm_vec{w + 3 * m * rw, nullptr, m + 1, 4 * b + 3, 0};
    }
    v[4 * B] = rs_msm_vec{dZ, zkinds.data(), m + 1, 4 * B, 1};
    msm_run(ctx, crs, 2, m + 1, v, NG, NG, mo, nullptr, used, st, pk->window, nullptr, pk->host_key != 0, pub, true);
  }
  size_t used_f[RS_MAX_BATCH] = {0};
  if (n_aux) {  // one pass over beta_prods for every member's F
    const uint64_t *crs[1] = {pk->d_beta_prods};
    rs_msm_vec v[RS_MAX_BATCH];
    for (int b = 0; b < B; b++)
      v[b] = rs_msm_vec{d_assignments[b] + cs->n_inputs * rw,
                        h_assignment_kinds ? h_assignment_kinds + (size_t)b * cs->n_vars + cs->n_inputs : nullptr, n_aux, b, 0};
    msm_run(ctx, crs, 1, n_aux, v, B, B, fb, nullptr, used_f, st, pk->window, nullptr, pk->host_key != 0, pub ? pub + 2 : nullptr, true);
  }
  auto slot = [&](int c, int g) { return mo + ((size_t)c * NG + g) * ew; };
  auto add_scaled = [&](uint64_t *dst, int *dst_empty, const uint64_t *enc, const uint64_t *d) {  // as in rinocchio_prove_run
    rs_msm_vec v{d, nullptr, 1, 0};
    const uint64_t *crs[1] = {enc};
    const uint64_t *add[1] = {*dst_empty ? nullptr : dst};
    msm_run(ctx, crs, 1, 1, &v, 1, 1, *dst_empty ? dst : tmp, add, nullptr, st, 0);
    if (!*dst_empty) RS_HIP(hipMemcpyAsync(dst, tmp, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    *dst_empty = 0;
  };
  for (int b = 0; b < B; b++) {  // the per-member epilogue of rinocchio_prove_run
    uint64_t *proof = d_proofs + (size_t)9 * b * ew;
    int empty[9];
    for (int k = 0; k < 4; k++) {
      empty[2 * k] = empty[2 * k + 1] = used[4 * b + k] == 0;
      RS_HIP(hipMemcpyAsync(proof + (size_t)(2 * k) * ew, slot(0, 4 * b + k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      RS_HIP(hipMemcpyAsync(proof + (size_t)(2 * k + 1) * ew, slot(1, 4 * b + k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    }
    if (zk)
      for (int k = 0; k < 3; k++) {
        add_scaled(proof + (size_t)(2 * k) * ew, &empty[2 * k], slot(0, 4 * B), dk(b, k));
        add_scaled(proof + (size_t)(2 * k + 1) * ew, &empty[2 * k + 1], slot(1, 4 * B), dk(b, k));
      }
    empty[8] = 1;
    uint64_t *F = proof + 8 * ew;
    if (n_aux) {
      RS_HIP(hipMemcpyAsync(F, fb + (size_t)b * ew, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      empty[8] = used_f[b] == 0;
      if (zk) {
        add_scaled(F, &empty[8], pk->d_beta_rv_ts, dk(b, 0));
        add_scaled(F, &empty[8], pk->d_beta_rw_ts, dk(b, 1));
        add_scaled(F, &empty[8], pk->d_beta_ry_ts, dk(b, 2));
      }
    } else {
      RS_HIP(hipMemsetAsync(F, 0, ew * sizeof(uint64_t), st));
    }
    if (h_empty) memcpy(h_empty + 9 * b, empty, sizeof(empty));
  }
  pt.mark(2);
  pt.finish();
  RS_HIP(hipStreamSynchronize(st));  // zkinds is a host temporary referenced by async copies
}

// workspace bytes of a batched proof (batch.h): the slots grow to the largest request of the passes
static size_t prove_batch_bytes(rs_ctx *ctx, const rs_r1cs *cs, int scheme, int batch) {
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words(), n_aux = cs->n_vars - cs->n_inputs;
  const size_t B = (size_t)batch;
  struct Pass {
    int n_crs, n_groups;
    size_t Tmax, used_words;
  };
  std::vector<Pass> passes;
  size_t bytes = 0;
  if (scheme == 0) {
    bytes += B * (5 * m + 1) * rw * sizeof(uint64_t) + 4 * B * ew * sizeof(uint64_t);
    passes.push_back({1, 2 * batch, m, 0});
    if (n_aux) passes.push_back({1, batch, n_aux, B * n_aux});
    passes.push_back({1, batch, m + 1, B * (m + 1)});
  } else {
    bytes += B * (4 * m + 1) * rw * sizeof(uint64_t) + (2 * (4 * B + 1) + B + 1) * ew * sizeof(uint64_t);
    passes.push_back({2, 4 * batch + 1, m + 1, B * (4 * m + 1) + m + 1});
    if (n_aux) passes.push_back({1, batch, n_aux, B * n_aux});
    bytes += m + 1;  // the kinds of Z
  }
  size_t rows = 0, partial = 0, used = 0;
  for (const Pass &p : passes) {
    const MsmGeometry g = msm_geometry(ctx, p.n_crs, p.n_groups, p.Tmax, 0, false, false, true);
    rows = std::max(rows, std::max<size_t>(256, g.tile_terms * (size_t)p.n_groups * ctx->L * ctx->N_enc * sizeof(double)));
    partial = std::max(partial, (size_t)g.n_chunks * p.n_crs * p.n_groups * ew * sizeof(uint64_t));
    used = std::max(used, p.used_words * sizeof(unsigned));
  }
  return bytes + rows + partial + used + B * n_aux;  // + the wire kinds of every member's auxiliary wires
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_groth16_prove(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, const uint64_t *d_assignment,
                     uint64_t *d_proof, int *h_empty, rs_stream stream) {
  return rs_groth16_prove_kinds(ctx, cs, pk, d_assignment, nullptr, d_proof, h_empty, stream);
}

int rs_groth16_prove_kinds(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, const uint64_t *d_assignment,
                           const uint8_t *h_assignment_kinds, uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  groth16_prove_run(ctx, cs, pk, nullptr, d_assignment, h_assignment_kinds, d_proof, h_empty, S(stream));
  RS_API_END
}

int rs_rinocchio_prove(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, const uint64_t *d_assignment,
                       const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3, uint64_t *d_proof, int *h_empty,
                       rs_stream stream) {
  return rs_rinocchio_prove_kinds(ctx, cs, pk, d_assignment, nullptr, d_d1, d_d2, d_d3, d_proof, h_empty, stream);
}

int rs_rinocchio_prove_kinds(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, const uint64_t *d_assignment,
                             const uint8_t *h_assignment_kinds, const uint64_t *d_d1, const uint64_t *d_d2, const uint64_t *d_d3,
                             uint64_t *d_proof, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  rinocchio_prove_run(ctx, cs, pk, nullptr, d_assignment, h_assignment_kinds, d_d1, d_d2, d_d3, d_proof, h_empty, S(stream));
  RS_API_END
}

int rs_groth16_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, int batch, const uint64_t *const *d_assignments,
                           const uint8_t *h_assignment_kinds, uint64_t *d_proofs, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  groth16_prove_batch_run(ctx, cs, pk, nullptr, batch, d_assignments, h_assignment_kinds, d_proofs, h_empty, S(stream));
  RS_API_END
}

int rs_rinocchio_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, int batch, const uint64_t *const *d_assignments,
                             const uint8_t *h_assignment_kinds, const uint64_t *d_d123, uint64_t *d_proofs, int *h_empty,
                             rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  rinocchio_prove_batch_run(ctx, cs, pk, nullptr, batch, d_assignments, h_assignment_kinds, d_d123, d_proofs, h_empty, S(stream));
  RS_API_END
}

int rs_prove_batch_bytes(rs_ctx *ctx, const rs_r1cs *cs, int scheme, int batch, size_t *h_bytes) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(cs && h_bytes && (scheme == 0 || scheme == 1), "bad argument");
  RS_REQUIRE(batch >= 1 && batch <= RS_MAX_BATCH, "batch must be in the range 1.." + std::to_string(RS_MAX_BATCH));
  *h_bytes = prove_batch_bytes(ctx, cs, scheme, batch);
  RS_API_END
}

int rs_fill_uniform(rs_ctx *ctx, uint64_t *d_dst, size_t count, int layout, uint64_t seed, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_dst && (layout == 0 || layout == 1), "bad argument");
  const size_t words = count * (layout == 0 ? ctx->ring_words() : ctx->enc_words());
  if (words) {
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 256 * 32);
    if (layout == 0)
      hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, S(stream), d_dst, words, (size_t)ctx->N, ctx->L,
                         ctx->d_qint, seed);
    else
      hipLaunchKernelGGL(fill_uniform_kernel, dim3(blocks), dim3(256), 0, S(stream), d_dst, words, (size_t)ctx->N_enc,
                         ctx->K, ctx->d_Qint, seed);
    RS_HIP(hipGetLastError());
  }
  RS_API_END
}

int rs_chain_assignment(rs_ctx *ctx, uint64_t *d_assignment, size_t m, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_assignment, "null argument");
  const size_t S_ = ctx->ring_words();
  if (ctx->use_int)
    hipLaunchKernelGGL(chain_kernel<ModI>, dim3((unsigned)((S_ + 255) / 256)), dim3(256), 0, S(stream), d_assignment, m, ctx->N,
                       ctx->L, ctx->d_qmod_i);
  else
    hipLaunchKernelGGL(chain_kernel<Mod>, dim3((unsigned)((S_ + 255) / 256)), dim3(256), 0, S(stream), d_assignment, m, ctx->N,
                       ctx->L, ctx->d_qmod);
  RS_HIP(hipGetLastError());
  RS_API_END
}

}  // extern "C"
