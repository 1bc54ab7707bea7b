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

// ---- One body per scheme proves the `B` members of a call: the witness map of every member into its slice of WS_PROVER_VECS,
// then ONE inner-product pass per key vector with the members' vectors as groups, so that a tile of the key is copied /
// expanded once.  The single-proof entry points call with one member and batched == false, the entry points of
// include/ringsnark_amd/batch.h with batched == true, whatever B: they ask msm_run for wide blocks (rs_prove_batch_bytes at
// batch 1 is sized for that) and take the inner products from WS_PROVER_OUT, where a single proof's land in the proof.

// One inner-product pass of a proof: an msm_run over n_keys key vectors with n_groups groups.
struct ProvePass {
  int n_keys, n_groups;
  size_t T;                       // terms of the longest vector; 0: the pass does not run (no auxiliary wires)
  size_t used_words, kind_bytes;  // of WS_MSM_USED when the pass counts the used terms, of WS_MSM_KINDS when every member gives kinds
};
// What a proof of B members takes: one member's words of WS_PROVER_VECS, the encoding elements of WS_PROVER_OUT, and the
// passes in the order they run.  The bodies and rs_prove_batch_bytes size their requests by it.
struct ProveLayout {
  size_t vec_words, out_elems;
  int n_pass;
  ProvePass pass[3];
};
static ProveLayout prove_layout(const rs_ctx *ctx, const rs_r1cs *cs, int scheme, int B) {
  const size_t m = cs->m, n_aux = cs->n_vars - cs->n_inputs, b = (size_t)B;
  const ProvePass aux{1, B, n_aux, b * n_aux, b * n_aux};  // a key vector over the members' auxiliary wires, as the caller holds them
  if (scheme == 0)  // vectors A_io, A_mid, B_io, B_mid [m], H [m + 1]; outputs [B][2] (A_b, B_b), [B] <delta_mid, aux_b>, [B] C_b
    return {(5 * m + 1) * ctx->ring_words(), 4 * b, 3, {{1, 2 * B, m, 0, 0}, aux, {1, B, m + 1, b * (m + 1), 0}}};
  // vectors A_mid, B_mid, C_mid [m], H [m + 1]; outputs [2][4 B + 1] (groups a_b, b_b, c_b, h_b per member, then Z, which every
  // member shares), [B] <beta_prods, aux_b>, one temporary
  return {(4 * m + 1) * ctx->ring_words(), 2 * (4 * b + 1) + b + 1, 2, {{2, 4 * B + 1, m + 1, b * (4 * m + 1) + m + 1, m + 1}, aux, {}}};
}

// The key vectors of a proving key in the order of the public seeds `pub` of a seeded one (nullptr: a full key); packed: the
// mark of packed.h beside them
struct ProverKey {
  const uint64_t *vecs[3];
  const uint64_t *pub;
  size_t window;
  bool on_host, packed;
  // vectors k .. k + n - 1, of len elements, as the key side of a pass
  MsmKey at(int k, int n, size_t len) const { return MsmKey{vecs + k, n, len, window, on_host, pub ? pub + k : nullptr, packed}; }
};

static void require_members(int batch, const uint64_t *const *d_assignments, bool batched) {
  RS_REQUIRE(batch >= 1 && batch <= RS_MAX_BATCH, "batch must be in the range 1.." + std::to_string(RS_MAX_BATCH));
  RS_REQUIRE(batched || batch == 1, "a single-proof entry point proves one member");
  RS_REQUIRE(d_assignments != nullptr, "null argument");
  for (int b = 0; b < batch; b++) RS_REQUIRE(d_assignments[b] != nullptr, batched ? "null assignment in the batch" : "null argument");
}

// groth16::prover (groth16.tcc:70-115).  pub: nullptr, or the public seeds of s_pows, delta_ts, delta_mid of a seeded key.
// h_kinds: nullptr or [B][n_vars]; d_proofs [B][3], h_empty nullptr or [B][3].
void groth16_prove_members(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, const uint64_t *pub, int B,
                           const uint64_t *const *d_assignments, const uint8_t *h_kinds, uint64_t *d_proofs, int *h_empty, bool batched,
                           hipStream_t st, bool packed) {
  require_members(B, d_assignments, batched);
  RS_REQUIRE(ctx && cs && pk && d_proofs, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_delta_ts && pk->d_alpha && pk->d_beta, "incomplete proving key");
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  RS_REQUIRE(n_aux == 0 || pk->d_delta_mid, "delta_mid missing");
  WsScope ws_scope(ctx, st);
  const ProveLayout lay = prove_layout(ctx, cs, 0, B);
  const ProverKey key{{pk->d_s_pows, pk->d_delta_ts, pk->d_delta_mid}, pub, pk->window, pk->host_key != 0, packed};
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  // witness map (groth16.tcc:82-84: d1 = d2 = d3 = 0); C_io / C_mid are not consumed by the prover
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (size_t)B * lay.vec_words * sizeof(uint64_t));
  auto A_io = [&](int b) { return wbuf + (size_t)b * lay.vec_words; };
  auto A_mid = [&](int b) { return A_io(b) + m * rw; };
  auto B_io = [&](int b) { return A_io(b) + 2 * m * rw; };
  auto B_mid = [&](int b) { return A_io(b) + 3 * m * rw; };
  auto H = [&](int b) { return A_io(b) + 4 * m * rw; };
  // The io vectors are linear forms of the primary inputs (witness.hip): when the inner product can take them in that
  // form (MsmLin) they are neither written by the witness map nor read and transformed by the inner product.
  const size_t nk = cs->n_inputs + 1;  // [1, x_1 .. x_n_inputs]; their encodings are staged in the (then unused) io rows
  const bool lin = g_tune.prover_lin_io && msm_supports_lin(ctx) && witness_io_shortcut(cs) &&
                   nk * std::max<size_t>(rw, (size_t)ctx->L * ctx->N_enc) <= m * rw;
  for (int b = 0; b < B; b++) {  // the plan is shared; the maps run one after another
    uint64_t *outs[7] = {lin ? nullptr : A_io(b), lin ? nullptr : B_io(b), nullptr, A_mid(b), B_mid(b), nullptr, H(b)};
    witness_run(ctx, cs, d_assignments[b], nullptr, nullptr, nullptr, outs, nullptr, st);
  }
  pt.mark(1);
  // Where the inner products land: [B][2] (A_b, B_b), [B] <delta_mid, aux_b>, [B] C_b.  A single proof's land in the proof
  // itself, C on top of <delta_mid, aux>; a batch's in WS_PROVER_OUT, from where every member's are copied into its proof.
  uint64_t *ab = d_proofs, *cmid = d_proofs + 2 * ew, *cfin = cmid;
  if (batched) {
    ab = (uint64_t *)ws_get(ctx, WS_PROVER_OUT, lay.out_elems * ew * sizeof(uint64_t));
    cmid = ab + (size_t)2 * B * ew;
    cfin = cmid + (size_t)B * ew;
  }
  {  // A_b = <s_pows, A_io> + <s_pows, A_mid> + alpha ; B_b likewise with beta   (groth16.tcc:89-103)
    const ProvePass &p = lay.pass[0];
    const uint64_t *add[2 * RS_MAX_BATCH];
    MsmLin ln[2 * RS_MAX_BATCH];
    rs_msm_vec v[4 * RS_MAX_BATCH];
    int nv = 0;
    for (int b = 0; b < B; b++) {
      add[2 * b] = pk->d_alpha;
      add[2 * b + 1] = pk->d_beta;
      if (lin) {
        // plaintexts of member b's [1, x_1 .. x_n_inputs]: (n_inputs + 1) batch encodings, staged in ITS unused io rows
        uint64_t *rings = A_io(b), *P = B_io(b);  // [nk][L][N] and [nk][L][N_enc] words
        fill_ones(ctx, rings, rw, st);
        if (cs->n_inputs) RS_HIP(hipMemcpyAsync(rings + rw, d_assignments[b], cs->n_inputs * rw * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        batch_encode_run(ctx, rings, P, nk, st);
        for (int w = 0; w < 2; w++) ln[2 * b + w] = MsmLin{cs->d_io_k[w], cs->d_io_c[w], cs->io_count[w], cs->d_io_cols, cs->io_M, P, m};
      }
      if (!lin) v[nv++] = rs_msm_vec{A_io(b), nullptr, p.T, 2 * b, 0};
      v[nv++] = rs_msm_vec{A_mid(b), nullptr, p.T, 2 * b, 0};
      if (!lin) v[nv++] = rs_msm_vec{B_io(b), nullptr, p.T, 2 * b + 1, 0};
      v[nv++] = rs_msm_vec{B_mid(b), nullptr, p.T, 2 * b + 1, 0};
    }
    msm_run(ctx, key.at(0, p.n_keys, m + 1), v, nv, p.n_groups, ab, add, nullptr, st, lin ? ln : nullptr, batched);
  }
  // C_b = <delta_ts, H_b> (+ <delta_mid, aux_b>)                           (groth16.tcc:105-112)
  size_t used_h[RS_MAX_BATCH], used_aux[RS_MAX_BATCH];
  for (int b = 0; b < B; b++) {
    used_h[b] = 1;
    used_aux[b] = 0;
  }
  rs_msm_vec v[RS_MAX_BATCH];
  if (const ProvePass &p = lay.pass[1]; p.T) {
    // the wires as the caller holds them: a Scalar-1 wire passes its key element through (seal_ring.tcc:525-527)
    for (int b = 0; b < B; b++)
      v[b] = rs_msm_vec{d_assignments[b] + cs->n_inputs * rw, h_kinds ? h_kinds + (size_t)b * cs->n_vars + cs->n_inputs : nullptr, p.T, b, 0};
    msm_run(ctx, key.at(2, p.n_keys, n_aux), v, B, p.n_groups, cmid, nullptr, h_empty ? used_aux : nullptr, st, nullptr, batched);
  }
  {
    const ProvePass &p = lay.pass[2];
    const uint64_t *add[RS_MAX_BATCH];
    for (int b = 0; b < B; b++) {
      v[b] = rs_msm_vec{H(b), nullptr, p.T, b, 0};
      add[b] = n_aux ? cmid + (size_t)b * ew : nullptr;
    }
    msm_run(ctx, key.at(1, p.n_keys, m + 1), v, B, p.n_groups, cfin, add, h_empty ? used_h : nullptr, st, nullptr, batched);
  }
  for (int b = 0; batched && b < B; b++) {
    uint64_t *proof = d_proofs + (size_t)3 * b * ew;
    RS_HIP(hipMemcpyAsync(proof, ab + (size_t)2 * b * ew, 2 * ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    RS_HIP(hipMemcpyAsync(proof + 2 * ew, cfin + (size_t)b * ew, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  pt.mark(2);
  pt.finish();
  if (key.on_host || h_kinds) RS_HIP(hipStreamSynchronize(st));  // the caller may release or rewrite the host key / the kinds on return
  if (h_empty)
    for (int b = 0; b < B; b++) {
      h_empty[3 * b] = h_empty[3 * b + 1] = 0;  // alpha / beta are always added
      h_empty[3 * b + 2] = (used_h[b] == 0 && used_aux[b] == 0) ? 1 : 0;
    }
}

// rinocchio::prover (rinocchio.tcc:75-190).  pub: nullptr, or the public seeds of s_pows, alpha_s_pows, beta_prods.
// d: d1, d2, d3 of member 0, all null for a proof that is not zero knowledge; member b's lie 3 b ring elements further (the
// [B][3] array of batch.h).  h_kinds: nullptr or [B][n_vars]; d_proofs [B][9], h_empty nullptr or [B][9].
void rinocchio_prove_members(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, const uint64_t *pub, int B,
                             const uint64_t *const *d_assignments, const uint8_t *h_kinds, const uint64_t *const d[3], uint64_t *d_proofs,
                             int *h_empty, bool batched, hipStream_t st, bool packed) {
  require_members(B, d_assignments, batched);
  RS_REQUIRE(ctx && cs && pk && d_proofs, "null argument");
  RS_REQUIRE(pk->d_s_pows && pk->d_alpha_s_pows, "incomplete proving key");
  RS_REQUIRE((d[0] && d[1] && d[2]) || (!d[0] && !d[1] && !d[2]), "d1,d2,d3 must be all set or all null");
  const size_t m = cs->m, rw = ctx->ring_words(), ew = ctx->enc_words();
  const size_t n_aux = cs->n_vars - cs->n_inputs;
  const bool zk = d[0] != nullptr;  // rinocchio.tcc:81-90
  RS_REQUIRE(n_aux == 0 || pk->d_beta_prods, "beta_prods missing");
  RS_REQUIRE(!zk || n_aux == 0 || (pk->d_beta_rv_ts && pk->d_beta_rw_ts && pk->d_beta_ry_ts), "beta_r*_ts missing");
  WsScope ws_scope(ctx, st);
  const ProveLayout lay = prove_layout(ctx, cs, 1, B);
  const ProverKey key{{pk->d_s_pows, pk->d_alpha_s_pows, pk->d_beta_prods}, pub, pk->window, pk->host_key != 0, packed};
  const int NG = lay.pass[0].n_groups;
  auto dk = [&](int b, int k) { return zk ? d[k] + (size_t)3 * b * rw : nullptr; };
  memset(&ctx->timings, 0, sizeof(ctx->timings));
  PhaseTimer pt(ctx, st);
  pt.mark(0);
  uint64_t *wbuf = (uint64_t *)ws_get(ctx, WS_PROVER_VECS, (size_t)B * lay.vec_words * sizeof(uint64_t));
  auto vec = [&](int b, int k) { return wbuf + (size_t)b * lay.vec_words + (size_t)k * m * rw; };  // A_mid, B_mid, C_mid, H of member b
  for (int b = 0; b < B; b++) {
    uint64_t *outs[7] = {nullptr, nullptr, nullptr, vec(b, 0), vec(b, 1), vec(b, 2), vec(b, 3)};
    witness_run(ctx, cs, d_assignments[b], dk(b, 0), dk(b, 1), dk(b, 2), outs, nullptr, st);
  }
  // coefficients_for_Z are slot constant: they go to the inner products as the compact [m+1][L] array of their values
  // (rs_msm_vec::slot_const) -- round 3 materialised m + 1 ring elements for them (a fifth of the prover's vectors).
  // A constant of the (context, m) plan: cached on the device, no host transpose and no synchronisation inside the proof.
  const uint64_t *dZ = witness_Z_rows(ctx, m);
  pt.mark(1);
  // [2][NG] inner products, [B] <beta_prods, aux_b>, one temporary
  uint64_t *mo = (uint64_t *)ws_get(ctx, WS_PROVER_OUT, lay.out_elems * ew * sizeof(uint64_t));
  uint64_t *fb = mo + (size_t)2 * NG * ew, *tmp = fb + (size_t)B * ew;
  std::vector<uint8_t> zkinds(m + 1, RS_KIND_POLY);
  zkinds[m] = RS_KIND_ONE;  // leading coefficient of Z is the RingElem Scalar 1 (evaluation_domain.tcc:55-58)
  size_t used[4 * RS_MAX_BATCH + 1] = {0}, used_f[RS_MAX_BATCH] = {0};
  rs_msm_vec v[4 * RS_MAX_BATCH + 1];
  {  // the ten inner products of rinocchio.tcc:106-163 of every member in one grouped pass over both key vectors
    const ProvePass &p = lay.pass[0];
    for (int b = 0; b < B; b++)
      for (int k = 0; k < 4; k++) v[4 * b + k] = rs_msm_vec{vec(b, k), nullptr, k < 3 ? m : m + 1, 4 * b + k, 0};
    v[4 * B] = rs_msm_vec{dZ, zkinds.data(), p.T, 4 * B, 1};
    msm_run(ctx, key.at(0, p.n_keys, m + 1), v, NG, p.n_groups, mo, nullptr, used, st, nullptr, batched);
  }
  if (const ProvePass &p = lay.pass[1]; p.T) {  // <beta_prods, aux_b>: a single proof's lands in its F, a batch's in WS_PROVER_OUT
    for (int b = 0; b < B; b++)
      v[b] = rs_msm_vec{d_assignments[b] + cs->n_inputs * rw, h_kinds ? h_kinds + (size_t)b * cs->n_vars + cs->n_inputs : nullptr, p.T, b, 0};
    msm_run(ctx, key.at(2, p.n_keys, n_aux), v, B, p.n_groups, batched ? fb : d_proofs + 8 * ew, nullptr, used_f, st, nullptr, batched);
  }
  auto slot = [&](int c, int g) { return mo + ((size_t)c * NG + g) * ew; };
  auto add_scaled = [&](uint64_t *dst, int *dst_empty, const uint64_t *enc, const uint64_t *d_ring) {
    // dst += d_ring * enc   (RingT * EncT then +=, rinocchio.tcc:168-173, 181-183)
    rs_msm_vec sv{d_ring, nullptr, 1, 0};
    const uint64_t *crs[1] = {enc};
    const uint64_t *add[1] = {*dst_empty ? nullptr : dst};
    msm_run(ctx, MsmKey{crs, 1, 1, 0}, &sv, 1, 1, *dst_empty ? dst : tmp, add, nullptr, st);
    if (!*dst_empty) RS_HIP(hipMemcpyAsync(dst, tmp, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    *dst_empty = 0;
  };
  for (int b = 0; b < B; b++) {
    uint64_t *proof = d_proofs + (size_t)9 * b * ew;
    int empty[9];
    for (int k = 0; k < 4; k++) {
      empty[2 * k] = empty[2 * k + 1] = used[4 * b + k] == 0;
      RS_HIP(hipMemcpyAsync(proof + (size_t)(2 * k) * ew, slot(0, 4 * b + k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      RS_HIP(hipMemcpyAsync(proof + (size_t)(2 * k + 1) * ew, slot(1, 4 * b + k), ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    }
    if (zk)  // rinocchio.tcc:167-174
      for (int k = 0; k < 3; k++) {
        add_scaled(proof + (size_t)(2 * k) * ew, &empty[2 * k], slot(0, 4 * B), dk(b, k));
        add_scaled(proof + (size_t)(2 * k + 1) * ew, &empty[2 * k + 1], slot(1, 4 * B), dk(b, k));
      }
    // F (rinocchio.tcc:176-185)
    empty[8] = 1;
    uint64_t *F = proof + 8 * ew;
    if (n_aux) {
      if (batched) RS_HIP(hipMemcpyAsync(F, fb + (size_t)b * ew, ew * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
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
  const ProveLayout lay = prove_layout(ctx, cs, scheme, batch);
  const size_t ew = ctx->enc_words();
  size_t rows = 0, partial = 0, used = 0, kinds = 0;
  for (int i = 0; i < lay.n_pass; i++) {
    const ProvePass &p = lay.pass[i];
    if (!p.T) continue;
    const MsmGeometry g = msm_geometry(ctx, MsmKey{nullptr, p.n_keys, p.T, 0}, p.n_groups, p.T, true);
    rows = std::max(rows, std::max<size_t>(256, g.tile_terms * (size_t)p.n_groups * ctx->L * ctx->N_enc * sizeof(double)));
    partial = std::max(partial, (size_t)g.n_chunks * p.n_keys * p.n_groups * ew * sizeof(uint64_t));
    used = std::max(used, p.used_words * sizeof(unsigned));
    kinds += p.kind_bytes;
  }
  return ((size_t)batch * lay.vec_words + lay.out_elems * ew) * sizeof(uint64_t) + rows + partial + used + kinds;
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
  groth16_prove_members(ctx, cs, pk, nullptr, 1, &d_assignment, h_assignment_kinds, d_proof, h_empty, false, S(stream));
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
  const uint64_t *d[3] = {d_d1, d_d2, d_d3};
  rinocchio_prove_members(ctx, cs, pk, nullptr, 1, &d_assignment, h_assignment_kinds, d, d_proof, h_empty, false, S(stream));
  RS_API_END
}

int rs_groth16_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_groth16_pk *pk, int batch, const uint64_t *const *d_assignments,
                           const uint8_t *h_assignment_kinds, uint64_t *d_proofs, int *h_empty, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  groth16_prove_members(ctx, cs, pk, nullptr, batch, d_assignments, h_assignment_kinds, d_proofs, h_empty, true, S(stream));
  RS_API_END
}

int rs_rinocchio_prove_batch(rs_ctx *ctx, const rs_r1cs *cs, const rs_rinocchio_pk *pk, int batch, const uint64_t *const *d_assignments,
                             const uint8_t *h_assignment_kinds, const uint64_t *d_d123, uint64_t *d_proofs, int *h_empty,
                             rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  const size_t rw = ctx->ring_words();
  const uint64_t *d[3] = {d_d123, d_d123 ? d_d123 + rw : nullptr, d_d123 ? d_d123 + 2 * rw : nullptr};
  rinocchio_prove_members(ctx, cs, pk, nullptr, batch, d_assignments, h_assignment_kinds, d, d_proofs, h_empty, true, S(stream));
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
  dispatch_arith(ctx, [&](auto tag) {
    using M = decltype(tag);
    hipLaunchKernelGGL(chain_kernel<M>, dim3((unsigned)((S_ + 255) / 256)), dim3(256), 0, S(stream), d_assignment, m, ctx->N, ctx->L,
                       CtxArith<M>::qmod(ctx));
  });
  RS_HIP(hipGetLastError());
  RS_API_END
}

}  // extern "C"
