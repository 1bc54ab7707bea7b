// keygen.hip -- SURVEY.md section 8(f) row f3: groth16::generator (zk_proof_systems/groth16/groth16.tcc:5-66) and
// rinocchio::generator (zk_proof_systems/rinocchio/rinocchio.tcc:5-72) on the device.
//
// Every vector of a proving key is an encoding of a linear form of the instance map's rows,
//     key[t] = E( sum_{r < R} coef_r * row_r[t] ),   R <= 3,
// with coef_r ring elements that depend on the trapdoor only (beta delta^-1, Z(s) delta^-1, alpha, ...).  The instance map
// is the code behind rs_instance_map_eval, the coefficient elements come from rs_ring_inv / rs_ring_mul, and one kernel does
// the rest per (element, limb): the linear form slot by slot, the slot scatter and the inverse transform modulo the plain
// prime ONCE, then for each data prime Q_j one forward transform of lift(m) - t e.  The arithmetic is exact and the
// transform is linear, so NTT(lift(m)) - t NTT(e) = NTT(lift(m) - t e): the canonical residues are those of encode_kernel
// (encoding.hip), which runs K workgroups per (element, limb) and three transforms in each -- K + 1 transforms here, 3K there.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "../../include/ringsnark_amd/keygen.h"
#include "ntt_core.hpp"
#include "rs_internal.hpp"

namespace rs {

// at most three (coefficient, rows) pairs; coef[r] == nullptr: the coefficient is 1
struct LinRows {
  const uint64_t *coef[3];  // [L][N]
  const uint64_t *rows[3];  // [count][L][N]
  int R;
};

// centre(c) - e t as a residue of Q_j; c canonical mod t, e in {-1, 0, 1}
__device__ __forceinline__ double lift_minus_te(double c, int e, const Mod &tmod, const Mod &mod) {
  // |centre(c)| <= t / 2 < 2^49 and |e t| < 2^50: the difference is below 2^51, inside reduce's bound of 2^52
  return reduce(center(c, tmod) - (double)e * tmod.p, mod);
}
__device__ __forceinline__ uint64_t lift_minus_te(uint64_t c, int e, const ModI &tmod, const ModI &mod) {
  const uint64_t x = lift_residue(lift_centered(c, tmod), mod), tq = tmod.p % mod.p;
  return e > 0 ? subm(x, tq, mod) : (e < 0 ? addm(x, tq, mod) : x);
}

// One workgroup per (element, limb); PER = n / blockDim <= 16.  Stream layout of oracle/rs_oracle.c rso_encrypt_symmetric,
// as encode_kernel: draws 1..n are the ternary error (shared by the K primes), draw n + j*n + x + 1 is a_j[x].
// LDS: one tile of n values (128 KiB + padding at n = 16384: one workgroup per CU, no second buffer).
// pub0: the seed of the vector's PUBLIC stream, which a is drawn from (seeded.h; pub0 == seed0: the one stream of keygen.h).
// COMPACT: a seeded vector -- c1 is not stored and the elements are [L][K][n] words apart.
template <class M, bool COMPACT>
__global__ void __launch_bounds__(1024)
keygen_encode_kernel(LinRows lf, const uint64_t *__restrict__ sk, uint64_t *__restrict__ enc, uint64_t seed0, uint64_t pub0, int N, int L, int K,
                     int logn, const uint32_t *__restrict__ index_map,
                     const NttTableT<typename ArithOf<M>::T, M> *__restrict__ plain_tabs,
                     const NttTableT<typename ArithOf<M>::T, M> *__restrict__ coeff_tabs) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T *s = reinterpret_cast<T *>(smem);
  const int n = 1 << logn;
  const size_t el = blockIdx.x;
  const size_t elem = el / (size_t)L;
  const int limb = (int)(el % (size_t)L);
  const NttTableT<T, M> pt = plain_tabs[limb];
  const M tmod = pt.mod;
  const uint64_t seed = (seed0 + elem) * 1315423911ull + (uint64_t)limb + 1;  // rso_enc_encode's per-limb stream
  const uint64_t pseed = (pub0 + elem) * 1315423911ull + (uint64_t)limb + 1;
  // 1. the linear form per slot, scattered (BatchEncoder::encode)
  for (int p = threadIdx.x; p < n; p += blockDim.x) s[pidx(p)] = T(0);
  __syncthreads();
  for (int x = threadIdx.x; x < N; x += blockDim.x) {
    T acc = T(0);
    for (int r = 0; r < lf.R; r++) {
      const T row = from_res<T>(lf.rows[r][el * (size_t)N + x]);
      const T term = lf.coef[r] ? mulmod_dd(center(from_res<T>(lf.coef[r][(size_t)limb * N + x]), tmod), row, tmod) : row;
      acc = reduce(addm(acc, term, tmod), tmod);
    }
    s[pidx((int)index_map[x])] = canon(acc, tmod);
  }
  __syncthreads();
  // 2. one inverse transform modulo the plain prime; the scaled coefficients stay in registers
  lds_ntt_inv(s, logn, pt.d_itw, 1, tmod, FP ? pt.inv_red_mask : 0u);
  T C[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int p = threadIdx.x + k * blockDim.x;
    if (p < n) C[k] = canon(mulmod(reduce(s[pidx(p)], tmod), pt.ninv, tmod), tmod);
  }
  uint32_t E = 0;  // the ternary error of the element's stream, e + 1 in two bits per own coefficient
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int p = threadIdx.x + k * blockDim.x;
    if (p < n) E |= (uint32_t)(splitmix_at(seed, (uint64_t)p + 1) % 3) << (2 * k);
  }
  // 3. per data prime: one forward transform of lift(m) - t e
  for (int j = 0; j < K; j++) {
    const NttTableT<T, M> ct = coeff_tabs[j];
    const M mod = ct.mod;
    const uint64_t Q = modulus_u64(mod);
    __syncthreads();  // the tile's last readers (the scaling above, the stores of prime j - 1) are done
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int p = threadIdx.x + k * blockDim.x;
      if (p < n) s[pidx(p)] = lift_minus_te(C[k], (int)((E >> (2 * k)) & 3u) - 1, tmod, mod);
    }
    __syncthreads();
    lds_ntt_fwd(s, logn, ct.d_tw, 1, mod, FP ? ct.fwd_red_mask : 0u);
    uint64_t *c0 = enc + (el * (COMPACT ? 1 : 2) * K + j) * (size_t)n, *c1 = c0 + (size_t)K * n;
    const uint64_t *sj = sk + (size_t)j * n;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int p = threadIdx.x + k * blockDim.x;
      if (p < n) {
        const uint64_t a = splitmix_at(pseed, (uint64_t)n + (uint64_t)j * n + (uint64_t)p + 1) % Q;
        const T as = mulmod_dd(from_res<T>(a), from_res<T>(sj[p]), mod);
        if (!COMPACT) c1[p] = a;
        c0[p] = to_res(canon(subm(reduce(s[pidx(p)], mod), as, mod), mod));
      }
    }
  }
}

template <class M, bool COMPACT>
static void encode_linear_launch(rs_ctx *ctx, const LinRows &lf, const uint64_t *d_sk, size_t count, uint64_t seed, uint64_t pub,
                                 uint64_t *d_enc, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  if (count == 0) return;
  RS_REQUIRE(count * (size_t)ctx->L < ((size_t)1 << 31), "too many elements for one launch");
  const size_t lds = padded_len((size_t)ctx->N_enc) * sizeof(T);
  const int thr = std::max(enc_threads(ctx->logN_enc), ctx->N_enc / 16);  // as rs_enc_encode: at most 16 coefficients per thread
  set_max_dyn_lds((const void *)keygen_encode_kernel<M, COMPACT>, (int)lds);
  const double n = (double)ctx->N_enc, el = (double)count * ctx->L;
  // algorithmic bytes: the rows and the written encodings; transforms: K + 1 per (element, limb)
  ProfScope p(ctx, st, "keygen_encode", el * 8 * (lf.R * ctx->N + (COMPACT ? 1.0 : 2.0) * ctx->K * n), el * (ctx->K + 1) * ntt_fp64(n, ctx->logN_enc));
  hipLaunchKernelGGL((keygen_encode_kernel<M, COMPACT>), dim3((unsigned)(count * ctx->L)), dim3(thr), lds, st, lf, d_sk, d_enc, seed, pub, ctx->N,
                     ctx->L, ctx->K, ctx->logN_enc, ctx->d_index_map, CtxArith<M>::d_plain(ctx), CtxArith<M>::d_coeff(ctx));
  RS_HIP(hipGetLastError());
}

// pub: the seed of the public stream (== seed: keygen.h); compact: the seeded layout, c0 only
static void encode_linear(rs_ctx *ctx, const LinRows &lf, const uint64_t *d_sk, size_t count, uint64_t seed, uint64_t pub, bool compact,
                          uint64_t *d_enc, hipStream_t st) {
  dispatch_arith(ctx, [&](auto tag) {
    using M = decltype(tag);
    if (compact) encode_linear_launch<M, true>(ctx, lf, d_sk, count, seed, pub, d_enc, st);
    else encode_linear_launch<M, false>(ctx, lf, d_sk, count, seed, pub, d_enc, st);
  });
}

constexpr size_t KEYGEN_HOST_TILE = 64;  // elements per staging buffer of a host-resident key when the caller names none

// One vector of a key: `count` elements of the linear form lf (rows advance with the element), seeds seed + k.
// to_host: dst is a host pointer; tiles go through the two staging buffers, the copy of a tile on the copy stream under
// the kernel of the next one.  Ordering as msm_run's host-key tiles, the directions reversed: the copy stream waits for
// ev_encoded[buf] (the kernel filled the buffer), the kernel that refills the buffer waits for ev_drained[buf].
// pub, compact: as encode_linear; the tiles and copies of a compact vector are half the size.
// packed (with compact; packed.h): every tile of at most `tile` elements is encoded compact into the FIRST staging buffer and
// packed from there by pack_c0_kernel on `st` -- a device-resident vector straight into its place (it never exists
// unpacked), a host-resident one into a second pair of buffers behind the two compact ones, [2][tile] packed elements, which
// the copy stream drains under the same two events (ev_encoded: the tile is packed).  One compact buffer serves: the kernel
// that refills it follows the pack kernel that read it on `st`.
static void encode_vector(rs_ctx *ctx, LinRows lf, const uint64_t *d_sk, size_t count, uint64_t seed, uint64_t pub, bool compact,
                          bool packed, uint64_t *dst, bool to_host, size_t tile, uint64_t *stage, hipStream_t st) {
  if (packed) {
    KeygenState &kg = ctx->keygen;
    const size_t S = ctx->ring_words(), PW = packed_words(ctx);
    uint64_t *const pstage = stage + 2 * tile * (ctx->enc_words() / 2);
    int tile_idx = 0;
    for (size_t t0 = 0; t0 < count; t0 += tile, tile_idx++) {
      const int buf = tile_idx & 1;
      const size_t tt = std::min(tile, count - t0);
      LinRows part = lf;
      for (int r = 0; r < lf.R; r++) part.rows[r] = lf.rows[r] + t0 * S;
      encode_linear(ctx, part, d_sk, tt, seed + t0, pub + t0, true, stage, st);
      if (!to_host) {
        pack_c0_run(ctx, stage, tt, dst + t0 * PW, nullptr, st);
        continue;
      }
      uint64_t *d_tile = pstage + (size_t)buf * tile * PW;
      if (tile_idx >= 2) RS_HIP(hipStreamWaitEvent(st, kg.ev_drained[buf], 0));  // the copy of tile - 2 has left the buffer
      pack_c0_run(ctx, stage, tt, d_tile, nullptr, st);
      RS_HIP(hipEventRecord(kg.ev_encoded[buf], st));
      RS_HIP(hipStreamWaitEvent(kg.copy_stream, kg.ev_encoded[buf], 0));
      RS_HIP(hipMemcpyAsync(dst + t0 * PW, d_tile, tt * PW * sizeof(uint64_t), hipMemcpyDeviceToHost, kg.copy_stream));
      RS_HIP(hipEventRecord(kg.ev_drained[buf], kg.copy_stream));
    }
    if (to_host) RS_HIP(hipStreamSynchronize(kg.copy_stream));
    return;
  }
  if (!to_host) {
    encode_linear(ctx, lf, d_sk, count, seed, pub, compact, dst, st);
    return;
  }
  KeygenState &kg = ctx->keygen;
  const size_t S = ctx->ring_words(), EW = compact ? ctx->enc_words() / 2 : ctx->enc_words();
  int tile_idx = 0;
  for (size_t t0 = 0; t0 < count; t0 += tile, tile_idx++) {
    const int buf = tile_idx & 1;
    const size_t tt = std::min(tile, count - t0);
    LinRows part = lf;
    for (int r = 0; r < lf.R; r++) part.rows[r] = lf.rows[r] + t0 * S;
    uint64_t *d_tile = stage + (size_t)buf * tile * EW;
    if (tile_idx >= 2) RS_HIP(hipStreamWaitEvent(st, kg.ev_drained[buf], 0));  // the copy of tile - 2 has left the buffer
    encode_linear(ctx, part, d_sk, tt, seed + t0, pub + t0, compact, d_tile, st);
    RS_HIP(hipEventRecord(kg.ev_encoded[buf], st));
    RS_HIP(hipStreamWaitEvent(kg.copy_stream, kg.ev_encoded[buf], 0));
    RS_HIP(hipMemcpyAsync(dst + t0 * EW, d_tile, tt * EW * sizeof(uint64_t), hipMemcpyDeviceToHost, kg.copy_stream));
    RS_HIP(hipEventRecord(kg.ev_drained[buf], kg.copy_stream));
  }
  // the next vector starts at buffer 0 again: both buffers are free once the copy stream has drained
  RS_HIP(hipStreamSynchronize(kg.copy_stream));
}

// [a, a + la) and [b, b + lb) intersect modulo 2^64 (stream indices wrap as the kernel's seed + k does)
static bool ranges_meet(uint64_t a, uint64_t la, uint64_t b, uint64_t lb) {
  if (la == 0 || lb == 0) return false;
  return (uint64_t)(b - a) < la || (uint64_t)(a - b) < lb;
}

// Scratch of a generator call: one allocation, overwritten with zeros before it is freed (on every path).
struct SecretScratch {
  uint64_t *p = nullptr;
  size_t bytes = 0;
  hipStream_t st = nullptr;
  ~SecretScratch() {
    if (!p) return;
    (void)hipStreamSynchronize(st);
    (void)hipMemset(p, 0, bytes);
    (void)hipDeviceSynchronize();
    (void)hipFree(p);
  }
};

static void ring_op(int status) {
  if (status != RS_OK) throw Error(status, rs_last_error());
}

struct KeyVector {
  LinRows lf;
  size_t count;
  uint64_t *dst;
  bool big;  // one of the vectors that live on the host under host_key
};

// SCHEME 0: groth16 (trap = alpha, beta, delta), 1: rinocchio (trap = alpha, beta, r_v, r_w, r_y).
// dst: the scheme's outputs in the order of h_seeds.  h_pub != nullptr: a seeded key (seeded.h) -- the three vectors compact,
// a of every element from the public stream h_pub[v] + k; packed: those three vectors bit-packed (packed.h), tiled by `tile`
// wherever they live.
template <int SCHEME>
static void keygen_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *const *trap, const uint64_t *d_sk,
                       const uint64_t *h_seeds, const uint64_t *h_pub, uint64_t *const *dst, bool host_key, size_t tile, hipStream_t st,
                       bool packed) {
  constexpr int NV = SCHEME == 0 ? 5 : 6, NT = SCHEME == 0 ? 3 : 5;
  RS_REQUIRE(cs && d_s && d_sk && h_seeds, "null argument");
  for (int e = 0; e < NT; e++) RS_REQUIRE(trap[e] != nullptr, "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  RS_REQUIRE(cs->m >= 1 && cs->n_inputs <= cs->n_vars, "empty constraint system");
  RS_REQUIRE(ctx->N_enc <= 16 * 1024, "encoding degree out of range");
  const size_t m = cs->m, n1 = cs->n_vars + 1, n_aux = cs->n_vars - cs->n_inputs, S = ctx->ring_words();
  size_t len[NV];
  len[0] = len[1] = m + 1, len[2] = n_aux;
  for (int v = 3; v < NV; v++) len[v] = 1;
  for (int v = 0; v < NV; v++) RS_REQUIRE(dst[v] != nullptr || len[v] == 0, "null argument");
  for (int v = 0; v < NV; v++)
    for (int w = 0; w < v; w++)
      RS_REQUIRE(!ranges_meet(h_seeds[v], len[v], h_seeds[w], len[w]),
                 "seed ranges of two key vectors intersect: their elements would share the encryption randomness");
  if (h_pub)
    for (int v = 0; v < NV; v++)
      for (int w = 0; w < v; w++)
        RS_REQUIRE(!ranges_meet(h_pub[v], len[v], h_pub[w], len[w]),
                   "public seed ranges of two key vectors intersect: their elements would share the polynomial a");
  RS_REQUIRE(h_pub || !packed, "a packed key is a seeded key");
  if ((host_key || packed) && tile == 0) tile = KEYGEN_HOST_TILE;
  if (host_key || packed) RS_REQUIRE(tile * (size_t)ctx->L < ((size_t)1 << 31), "tile too large");

  // scratch: At, Bt, Ct [n1], Ht [m+1], Zt, and 7 coefficient elements
  SecretScratch sc;
  sc.st = st;
  sc.bytes = (3 * n1 + (m + 1) + 1 + 7) * S * sizeof(uint64_t);
  RS_HIP(hipMalloc(&sc.p, sc.bytes));
  uint64_t *At = sc.p, *Bt = At + n1 * S, *Ct = Bt + n1 * S, *Ht = Ct + n1 * S, *Zt = Ht + (m + 1) * S, *co = Zt + S;
  auto coef = [&](int k) { return co + (size_t)k * S; };
  rs_stream rst = (rs_stream)st;
  const uint64_t *alpha = trap[0], *beta = trap[1];
  if (SCHEME == 0) {  // delta must be a unit (groth16.tcc:21): found before anything else is computed
    ring_op(rs_ring_inv(ctx, coef(0), trap[2], 1, rst));  // delta^-1
  }
  instance_map_run(ctx, cs, d_s, At, Bt, Ct, Ht, Zt, st, true);  // throws for a domain element
  const size_t k0 = cs->n_inputs + 1;  // first auxiliary variable
  KeyVector vec[NV];
  auto rows1 = [](const uint64_t *c, const uint64_t *r) {
    LinRows l{};
    l.coef[0] = c, l.rows[0] = r, l.R = 1;
    return l;
  };
  auto rows3 = [&](const uint64_t *ca, const uint64_t *cb, const uint64_t *cc) {
    LinRows l{};
    l.coef[0] = ca, l.coef[1] = cb, l.coef[2] = cc;
    l.rows[0] = At + k0 * S, l.rows[1] = Bt + k0 * S, l.rows[2] = Ct + k0 * S;
    l.R = 3;
    return l;
  };
  vec[0] = {rows1(nullptr, Ht), m + 1, dst[0], true};
  if (SCHEME == 0) {
    const uint64_t *dinv = coef(0);
    ring_op(rs_ring_mul(ctx, coef(1), Zt, dinv, 1, rst));    // Z(s) delta^-1
    ring_op(rs_ring_mul(ctx, coef(2), beta, dinv, 1, rst));  // beta delta^-1
    ring_op(rs_ring_mul(ctx, coef(3), alpha, dinv, 1, rst)); // alpha delta^-1
    vec[1] = {rows1(coef(1), Ht), m + 1, dst[1], true};
    vec[2] = {rows3(coef(2), coef(3), dinv), n_aux, dst[2], true};
    vec[3] = {rows1(nullptr, alpha), 1, dst[3], false};
    vec[4] = {rows1(nullptr, beta), 1, dst[4], false};
  } else {
    for (int e = 0; e < 3; e++) ring_op(rs_ring_mul(ctx, coef(e), beta, trap[2 + e], 1, rst));  // beta r_v, beta r_w, beta r_y
    vec[1] = {rows1(alpha, Ht), m + 1, dst[1], true};
    vec[2] = {rows3(coef(0), coef(1), coef(2)), n_aux, dst[2], true};
    for (int e = 0; e < 3; e++) vec[3 + e] = {rows1(coef(e), Zt), 1, dst[3 + e], false};  // beta Z(s) r_*
  }
  {
    WsScope ws_scope(ctx, st);
    uint64_t *stage = nullptr;
    if (packed)  // the two compact buffers of a seeded key (the first is used), then [2][tile] packed elements for a host-resident key
      stage = (uint64_t *)ws_get(ctx, WS_KEYGEN_STAGE, 2 * tile * (ctx->enc_words() / 2 + (host_key ? packed_words(ctx) : 0)) * sizeof(uint64_t));
    if (host_key) {
      KeygenState &kg = ctx->keygen;
      if (!packed)
        stage = (uint64_t *)ws_get(ctx, WS_KEYGEN_STAGE, 2 * tile * (h_pub ? ctx->enc_words() / 2 : ctx->enc_words()) * sizeof(uint64_t));
      if (!kg.copy_stream) RS_HIP(hipStreamCreateWithFlags(&kg.copy_stream, hipStreamNonBlocking));
      for (int b = 0; b < 2; b++) {  // each by its own null test: a call that failed half way is completed by the next
        if (!kg.ev_encoded[b]) RS_HIP(hipEventCreateWithFlags(&kg.ev_encoded[b], hipEventDisableTiming));
        if (!kg.ev_drained[b]) RS_HIP(hipEventCreateWithFlags(&kg.ev_drained[b], hipEventDisableTiming));
      }
    }
    for (int v = 0; v < NV; v++)
      encode_vector(ctx, vec[v].lf, d_sk, vec[v].count, h_seeds[v], h_pub ? h_pub[v] : h_seeds[v], h_pub && vec[v].big, packed && vec[v].big,
                    vec[v].dst, host_key && vec[v].big, tile, stage, st);
    RS_HIP(hipStreamSynchronize(st));
  }
}


void keygen_run_scheme(int scheme, rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *const *trap, const uint64_t *d_sk,
                       const uint64_t *h_seeds, const uint64_t *h_pub, uint64_t *const *dst, bool host_key, size_t tile, hipStream_t st,
                       bool packed) {
  if (scheme == 0)
    keygen_run<0>(ctx, cs, d_s, trap, d_sk, h_seeds, h_pub, dst, host_key, tile, st, packed);
  else
    keygen_run<1>(ctx, cs, d_s, trap, d_sk, h_seeds, h_pub, dst, host_key, tile, st, packed);
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_groth16_keygen(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                      const uint64_t *d_delta, const uint64_t *d_sk, const uint64_t h_seeds[5], const rs_groth16_key_out *out,
                      rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr, "null argument");
  const uint64_t *trap[3] = {d_alpha, d_beta, d_delta};
  uint64_t *dst[5] = {out->s_pows, out->delta_ts, out->delta_mid, out->d_alpha, out->d_beta};
  keygen_run<0>(ctx, cs, d_s, trap, d_sk, h_seeds, nullptr, dst, out->host_key != 0, out->tile, S(stream), false);
  RS_API_END
}

int rs_rinocchio_keygen(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, const uint64_t *d_alpha, const uint64_t *d_beta,
                        const uint64_t *d_rv, const uint64_t *d_rw, const uint64_t *d_ry, const uint64_t *d_sk,
                        const uint64_t h_seeds[6], const rs_rinocchio_key_out *out, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(out != nullptr, "null argument");
  const uint64_t *trap[5] = {d_alpha, d_beta, d_rv, d_rw, d_ry};
  uint64_t *dst[6] = {out->s_pows, out->alpha_s_pows, out->beta_prods, out->d_beta_rv_ts, out->d_beta_rw_ts, out->d_beta_ry_ts};
  keygen_run<1>(ctx, cs, d_s, trap, d_sk, h_seeds, nullptr, dst, out->host_key != 0, out->tile, S(stream), false);
  RS_API_END
}

int rs_enc_encode_linear(rs_ctx *ctx, const uint64_t *d_sk, const uint64_t *const *d_coef, const uint64_t *const *d_rows,
                         int n_terms, size_t count, uint64_t seed, uint64_t *d_enc, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(d_sk && d_rows && d_enc, "null argument");
  RS_REQUIRE(n_terms >= 1 && n_terms <= 3, "a linear form has one to three terms");
  LinRows lf{};
  lf.R = n_terms;
  for (int r = 0; r < n_terms; r++) {
    RS_REQUIRE(d_rows[r] != nullptr, "null argument");
    lf.rows[r] = d_rows[r];
    lf.coef[r] = d_coef ? d_coef[r] : nullptr;
  }
  if (count == 0) return RS_OK;
  RS_REQUIRE(ctx->N_enc <= 16 * 1024, "encoding degree out of range");
  WsScope ws_scope(ctx, S(stream));
  encode_linear(ctx, lf, d_sk, count, seed, seed, false, d_enc, S(stream));
  RS_HIP(hipStreamSynchronize(S(stream)));
  RS_API_END
}

}  // extern "C"
