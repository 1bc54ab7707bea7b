// encoding.hip -- SURVEY.md section 8(f) rows f2 / f3: the two ends of the encoding scheme that sit
// either side of the prover.
//
//   rs_enc_decode   EncodingElem::decode  (ringsnark/seal/seal_ring.tcc:435-477): BGV decryption
//                   (c0 + c1*s -> coefficient form -> centred mod Q -> mod t) followed by
//                   BatchEncoder::decode (forward NTT mod t + slot gather).  What the verifier runs on
//                   the proof elements (groth16.tcc:118-121, rinocchio.tcc:203-214).
//   rs_enc_encode   EncodingElem::encode  (ringsnark/seal/seal_ring.tcc:324-359): BatchEncoder::encode
//                   + symmetric BGV encryption.  What the generator runs on every CRS element.
//
// Randomness: SEAL's sampler (Blake2xb / SHAKE, centred binomial) is not restated;
// the ciphertexts follow the CPU oracle's recipe (oracle/rs_oracle.c: splitmix64 stream, ternary
// error), which is all the parity tests can pin.  Any valid BGV ciphertext exercises the prover.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "ntt_core.hpp"
#include "rs_internal.hpp"

namespace rs {

// The kernels of this unit are written once on the vocabulary of intmod.hpp and instantiated for both arithmetics:
// M = Mod (exact FP64, lazy values) or ModI (contexts with a modulus >= 2^50: canonical residues, table constants in
// Montgomery form; mulmod = data x constant, mulmod_dd = data x data).

// ---- decode ----------------------------------------------------------------------------------
// v_j = iNTT_{Q_j}(c0 + c1 * s), canonical values.  grid (count * L, K)
template <class M>
__global__ void __launch_bounds__(1024)
decrypt_dot_kernel(const uint64_t *__restrict__ enc, const uint64_t *__restrict__ sk, typename ArithOf<M>::T *__restrict__ V, int K, int logn,
                   const NttTableT<typename ArithOf<M>::T, M> *__restrict__ coeff_tabs) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T *s = reinterpret_cast<T *>(smem);
  const int n = 1 << logn;
  const size_t el = blockIdx.x;  // (element, limb)
  const int j = blockIdx.y;
  const NttTableT<T, M> tab = coeff_tabs[j];
  const M mod = tab.mod;
  const uint64_t *c0 = enc + (el * 2 * K + j) * (size_t)n, *c1 = c0 + (size_t)K * n;
  const uint64_t *sj = sk + (size_t)j * n;
  for (int x = threadIdx.x; x < n; x += blockDim.x)
    s[pidx(x)] = addm(from_res<T>(c0[x]), mulmod_dd(from_res<T>(c1[x]), from_res<T>(sj[x]), mod), mod);
  __syncthreads();
  lds_ntt_inv(s, logn, tab.d_itw, 1, mod, FP ? tab.inv_red_mask : 0u);
  T *dst = V + (el * K + j) * (size_t)n;
  for (int x = threadIdx.x; x < n; x += blockDim.x) dst[x] = canon(mulmod(reduce(s[pidx(x)], mod), tab.ninv, mod), mod);
}

// Constants of the CRT composition (SEAL Decryptor::bgv_decrypt composes to the centred
// representative mod Q before reducing mod t): Garner mixed-radix digits, no big integers.
// What a kernel multiplies by is a table constant of the arithmetic (HostArith<M>::konst: balanced double / Montgomery
// form); what it adds, subtracts or compares is a plain canonical value (HostArith<M>::plain).
template <class M>
struct CrtConstsT {
  using T = typename ArithOf<M>::T;
  int K;
  M Qmod[RS_MAX_K];
  T half[RS_MAX_K];                 // mixed-radix digits of floor(Q/2), plain
  T prod_inv[RS_MAX_K];             // (prod_{i<k} Q_i)^-1 mod Q_k, constant
  T Qi_mod_Qk[RS_MAX_K][RS_MAX_K];  // [i][k] = Q_i mod Q_k, constant
};
template <class M>
struct CrtLimbT {
  using T = typename ArithOf<M>::T;
  M tmod;
  T Qk_mod_t[RS_MAX_K];  // constant
  T Q_mod_t;             // plain: the canonical residue in both arithmetics (it is subtracted, and the result reduced)
  T F;                   // constant: level factor prod_{j >= K} Q_j mod t of a decode below the context's level (modswitch.h)
  int scale;             // 0: the context's own level, F = 1 and no product is made
};

// ---- the noise guard of EncodingElem::decode (seal_ring.tcc:443-454) ----------------------------------------------
// SEAL 4.x Decryptor::invariant_noise_budget, scheme bgv (un-vendored dependency; its published algorithm): the noise
// polynomial is c0 + c1 s mod Q in coefficient form -- for BGV that IS m + t e, no scaling by the plain modulus (the
// multiplication by t is the BFV branch) -- CRT-composed, its infinity norm taken on the centred representatives, and
//     budget = max(0, bit_count(Q) - significant_bits(norm) - 1).
// The composition already runs here in mixed radix (digits d_k, value = d_0 + Q_0 (d_1 + Q_1 (...))), so the bit length
// of a centred magnitude is found WITHOUT big integers: thr[b][.] holds the digits of 2^b - 1 for b < bit_count(Q)
// (host, exact), |v| >= 2^b is a lexicographic digit comparison, and significant_bits(|v|) = #{b : |v| >= 2^b} by
// binary search (the predicate is monotone).  For v > floor(Q/2) the magnitude is Q - v = (Q - 1 - v) + 1 and
// Q - 1 - v has digits Q_k - 1 - d_k.
template <class T>
__device__ __forceinline__ int magnitude_bits(const T *d, bool upper, const T *Qk, const T *__restrict__ thr, int tb, int K) {
  T w[RS_MAX_K];
  for (int k = 0; k < K; k++) w[k] = upper ? Qk[k] - (T)1 - d[k] : d[k];
  int lo = 0, hi = tb;  // lo = number of b with |v| >= 2^b
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const T *t = thr + (size_t)mid * RS_MAX_K;
    int cmp = 0;
    for (int k = K - 1; k >= 0 && cmp == 0; k--) cmp = w[k] > t[k] ? 1 : (w[k] < t[k] ? -1 : 0);
    // lower half: |v| = w >= 2^b  <=>  w > 2^b - 1;   upper half: |v| = w + 1 >= 2^b  <=>  w >= 2^b - 1
    if (upper ? cmp >= 0 : cmp > 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// centred CRT composition mod t, forward NTT mod t, slot gather.  grid (count * L)
template <class M>
__global__ void __launch_bounds__(1024)
crt_decode_kernel(const typename ArithOf<M>::T *__restrict__ V, uint64_t *__restrict__ rings, int N, int L, int logn, CrtConstsT<M> cc,
                  const CrtLimbT<M> *__restrict__ limbs, const uint32_t *__restrict__ index_map,
                  const NttTableT<typename ArithOf<M>::T, M> *__restrict__ plain_tabs, const typename ArithOf<M>::T *__restrict__ thr, int tb,
                  int *__restrict__ noise_bits) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_bits;
  T *s = reinterpret_cast<T *>(smem);
  const int n = 1 << logn, K = cc.K;
  if (threadIdx.x == 0) s_bits = 0;
  __syncthreads();
  int my_bits = 0;
  T Qk[RS_MAX_K];
  for (int k = 0; k < K; k++) Qk[k] = cc.Qmod[k].p;
  const size_t el = blockIdx.x;
  const int limb = (int)(el % (size_t)L);
  const CrtLimbT<M> cl = limbs[limb];
  const NttTableT<T, M> tab = plain_tabs[limb];
  const M tmod = cl.tmod;
  const T *v = V + el * (size_t)K * n;
  for (int x = threadIdx.x; x < n; x += blockDim.x) {
    T d[RS_MAX_K];
    d[0] = v[x];
    for (int k = 1; k < K; k++) {  // value = d0 + Q0*(d1 + Q1*(d2 + ...))
      const M mk = cc.Qmod[k];
      T acc = T(0);
      for (int i = k - 1; i >= 0; i--) acc = reduce(addm(mulmod(acc, cc.Qi_mod_Qk[i][k], mk), digit_residue(d[i], mk), mk), mk);
      d[k] = canon(mulmod(reduce(subm(v[(size_t)k * n + x], acc, mk), mk), cc.prod_inv[k], mk), mk);
    }
    bool upper = false;  // value > floor(Q/2)?
    for (int k = K - 1; k >= 0; k--)
      if (d[k] != cc.half[k]) {
        upper = d[k] > cc.half[k];
        break;
      }
    my_bits = max(my_bits, magnitude_bits<T>(d, upper, Qk, thr, tb, K));
    T r = T(0);
    for (int k = K - 1; k >= 0; k--) r = reduce(addm(mulmod(r, cl.Qk_mod_t[k], tmod), digit_residue(d[k], tmod), tmod), tmod);
    if (upper) r = subm(r, cl.Q_mod_t, tmod);
    r = reduce(r, tmod);
    if (cl.scale) r = reduce(mulmod(r, cl.F, tmod), tmod);  // SEAL's correction_factor of a switched ciphertext
    s[pidx(x)] = r;
  }
  atomicMax(&s_bits, my_bits);
  __syncthreads();
  if (threadIdx.x == 0) noise_bits[el] = s_bits;  // significant bits of the infinity norm of this ciphertext's noise polynomial
  if (!rings) return;                              // rs_enc_noise_budget: the budget only
  lds_ntt_fwd(s, logn, tab.d_tw, 1, tmod, FP ? tab.fwd_red_mask : 0u);  // BatchEncoder::decode
  uint64_t *dst = rings + el * (size_t)N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = to_res(canon(s[pidx((int)index_map[i])], tmod));
}

// ---- encode ----------------------------------------------------------------------------------
// One workgroup per (element, limb, prime j): c1 = a, c0 = -(a*s + t*e) + NTT(lift(BatchEncode(ring limb))).
// Stream layout of oracle/rs_oracle.c rso_encrypt_symmetric: draws 1..n are the ternary error,
// draw n + j*n + x + 1 is a_j[x].  grid (count * L, K); PER = n / blockDim <= 16
template <class M>
__global__ void __launch_bounds__(1024)
encode_kernel(const uint64_t *__restrict__ rings, const uint64_t *__restrict__ sk, uint64_t *__restrict__ enc, uint64_t seed0,
              int N, int L, int K, int logn, const uint32_t *__restrict__ index_map,
              const NttTableT<typename ArithOf<M>::T, M> *__restrict__ plain_tabs,
              const NttTableT<typename ArithOf<M>::T, M> *__restrict__ coeff_tabs) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T *s = reinterpret_cast<T *>(smem);
  const int n = 1 << logn;
  const size_t el = blockIdx.x;
  const size_t elem = el / (size_t)L;
  const int limb = (int)(el % (size_t)L), j = blockIdx.y;
  const NttTableT<T, M> pt = plain_tabs[limb], ct = coeff_tabs[j];
  const M tmod = pt.mod, mod = ct.mod;
  const uint64_t t = modulus_u64(tmod), Q = modulus_u64(mod);
  const uint64_t seed = (seed0 + elem) * 1315423911ull + (uint64_t)limb + 1;  // rso_enc_encode's per-limb stream
  // BatchEncoder::encode: slot scatter + inverse NTT mod t
  for (int p = threadIdx.x; p < n; p += blockDim.x) s[pidx(p)] = T(0);
  __syncthreads();
  const uint64_t *src = rings + el * (size_t)N;
  for (int x = threadIdx.x; x < N; x += blockDim.x) s[pidx((int)index_map[x])] = from_res<T>(src[x]);
  __syncthreads();
  lds_ntt_inv(s, logn, pt.d_itw, 1, tmod, FP ? pt.inv_red_mask : 0u);
  // centred lift to Z_{Q_j} (in place; every thread touches only its own positions)
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    const T c = canon(mulmod(reduce(s[pidx(p)], tmod), pt.ninv, tmod), tmod);
    s[pidx(p)] = lift_residue(lift_centered(c, tmod), mod);
  }
  __syncthreads();
  lds_ntt_fwd(s, logn, ct.d_tw, 1, mod, FP ? ct.fwd_red_mask : 0u);
  T P[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int p = threadIdx.x + k * blockDim.x;
    if (p < n) P[k] = reduce(s[pidx(p)], mod);
  }
  __syncthreads();
  // ternary error, NTT form
  for (int p = threadIdx.x; p < n; p += blockDim.x) s[pidx(p)] = ternary_res((int)(splitmix_at(seed, (uint64_t)p + 1) % 3) - 1, mod);
  __syncthreads();
  lds_ntt_fwd(s, logn, ct.d_tw, 1, mod, FP ? ct.fwd_red_mask : 0u);
  const T tq = reduce(from_res<T>(t % Q), mod);
  uint64_t *c0 = enc + (el * 2 * K + j) * (size_t)n, *c1 = c0 + (size_t)K * n;
  const uint64_t *sj = sk + (size_t)j * n;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int p = threadIdx.x + k * blockDim.x;
    if (p < n) {
      const uint64_t a = splitmix_at(seed, (uint64_t)n + (uint64_t)j * n + (uint64_t)p + 1) % Q;
      const T as = mulmod_dd(from_res<T>(a), from_res<T>(sj[p]), mod);
      const T te = mulmod_dd(tq, reduce(s[pidx(p)], mod), mod);
      c1[p] = a;
      c0[p] = to_res(canon(subm(subm(P[k], as, mod), te, mod), mod));
    }
  }
}

// Host side of the noise guard: bit_count(Q) and the mixed-radix digits (radices Q_0, Q_1, ...) of 2^b - 1 for every
// b < bit_count(Q), by exact multi-word arithmetic (K <= 12 words of 62 bits).
struct BigU {
  uint64_t w[RS_MAX_K + 2];
  BigU() { memset(w, 0, sizeof(w)); }
  void mul_add(uint64_t m, uint64_t a) {  // this = this * m + a
    unsigned __int128 carry = a;
    for (int i = 0; i < RS_MAX_K + 2; i++) {
      const unsigned __int128 cur = (unsigned __int128)w[i] * m + carry;
      w[i] = (uint64_t)cur;
      carry = cur >> 64;
    }
  }
  uint64_t divmod(uint64_t dv) {  // this /= dv, returns the remainder
    unsigned __int128 rem = 0;
    for (int i = RS_MAX_K + 1; i >= 0; i--) {
      const unsigned __int128 cur = (rem << 64) | w[i];
      w[i] = (uint64_t)(cur / dv);
      rem = cur % dv;
    }
    return (uint64_t)rem;
  }
  int bits() const {
    for (int i = RS_MAX_K + 1; i >= 0; i--)
      if (w[i]) return 64 * i + 64 - __builtin_clzll(w[i]);
    return 0;
  }
};

// thr[b * RS_MAX_K + k] = digit k of 2^b - 1; returns bit_count(Q), Q the product of the first K primes
static int noise_thresholds(const rs_ctx *ctx, int K, std::vector<uint64_t> &thr) {
  BigU Q;
  Q.w[0] = 1;
  for (int k = 0; k < K; k++) Q.mul_add(ctx->Q[k], 0);
  const int tb = Q.bits();
  thr.assign((size_t)tb * RS_MAX_K, 0);
  for (int b = 0; b < tb; b++) {
    BigU v;  // 2^b - 1
    for (int i = 0; i < b / 64; i++) v.w[i] = ~0ull;
    if (b % 64) v.w[b / 64] = (1ull << (b % 64)) - 1;
    for (int k = 0; k < K; k++) thr[(size_t)b * RS_MAX_K + k] = v.divmod(ctx->Q[k]);
  }
  return tb;
}

}  // namespace rs

using namespace rs;

// rs::decode_impl (declared in rs_internal.hpp, defined below; modswitch.hip calls it too):
// EncodingElem::decode and Decryptor::invariant_noise_budget share everything up to the centred composition.
// d_rings == nullptr: budgets only.  h_budget [count * L] (may be null).  Throws RS_ERR_NOISE -- after writing every
// decoding -- when d_rings is given and a ciphertext has no budget left (seal_ring.tcc:446-454).  rs::decode_held is the same
// body for a caller that holds the context's lock and reads the verdict from h_budget instead (verify.hip).
// K: the level -- the first K primes of the context, d_enc [count][L][2][K][N_enc]; below ctx->K the decoding is
// multiplied by the level factor (modswitch.h).
extern "C" {

int rs_enc_decode(rs_ctx *ctx, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_sk && d_enc && d_rings, "null argument");
  return decode_impl(ctx, ctx->K, d_sk, d_enc, count, d_rings, nullptr, stream);
  RS_API_END
}

int rs_enc_noise_budget(rs_ctx *ctx, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, int *h_budget, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_sk && d_enc && h_budget, "null argument");
  return decode_impl(ctx, ctx->K, d_sk, d_enc, count, nullptr, h_budget, stream);
  RS_API_END
}

}  // extern "C"

// The guard's text for limb `limb` of element `element` of a decode of `count` elements: the reference's message
// (seal_ring.tcc:450-453; the budget it prints is max(0, .), i.e. 0), exactly, for one element (its decode takes one
// EncodingElem); a decode of several says which element it was.
std::string rs::noise_message(int limb, size_t element, size_t count) {
  return "ciphertext #" + std::to_string(limb) + " has remaining noise budget 0 <= 0" +
         (count > 1 ? " (element " + std::to_string(element) + " of the batch)" : std::string());
}

// the guard's verdict on the significant-bit counts the kernels found
static int noise_verdict(rs_ctx *ctx, const int *d_bits, size_t count, int tb, bool guard, int *h_budget) {
  std::vector<int> bits(count * (size_t)ctx->L);
  RS_HIP(hipMemcpy(bits.data(), d_bits, bits.size() * sizeof(int), hipMemcpyDeviceToHost));
  long long bad = -1;
  for (size_t e = 0; e < bits.size(); e++) {
    const int budget = std::max(0, tb - bits[e] - 1);  // "The -1 accounts for scaling the invariant noise by 2" (SEAL)
    if (h_budget) h_budget[e] = budget;
    if (budget <= 0 && bad < 0) bad = (long long)e;
  }
  if (guard && bad >= 0) throw rs::Error(RS_ERR_NOISE, noise_message((int)(bad % ctx->L), (size_t)(bad / ctx->L), count));
  return RS_OK;
}

// a table of constants that stays on the device for the life of the context
static void *upload_constants(const void *h, size_t bytes, const char *what) {
  void *p = nullptr;
  RS_HIP(hipMalloc(&p, bytes));
  if (hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    throw rs::Error(RS_ERR_HIP, std::string("upload of the ") + what + " failed");
  }
  return p;
}

// host constants of the CRT composition at level K
template <class M>
static CrtConstsT<M> crt_consts(const rs_ctx *ctx, int K) {
  using H = HostArith<M>;
  CrtConstsT<M> cc;
  memset(&cc, 0, sizeof(cc));
  cc.K = K;
  uint64_t carry = 0;
  for (int k = K - 1; k >= 0; k--) {  // digits of Q-1 are (Q_k - 1); halve from the top
    const unsigned __int128 cur = (unsigned __int128)(ctx->Q[k] - 1) + (unsigned __int128)carry * ctx->Q[k];
    cc.half[k] = H::plain((uint64_t)(cur >> 1), ctx->Q[k]);
    carry = (uint64_t)(cur & 1);
  }
  for (int k = 0; k < K; k++) {
    const uint64_t Qk = ctx->Q[k];
    cc.Qmod[k] = H::make(Qk);
    uint64_t prod = 1 % Qk;
    for (int i = 0; i < k; i++) prod = host::mulmod(prod, ctx->Q[i] % Qk, Qk);
    cc.prod_inv[k] = H::konst(k ? host::invmod(prod, Qk) : 1, Qk);
    for (int i = 0; i < K; i++) cc.Qi_mod_Qk[i][k] = H::konst(ctx->Q[i] % Qk, Qk);
  }
  return cc;
}

// ... and its per-limb constants (uploaded once per level: decode_arith)
template <class M>
static std::vector<CrtLimbT<M>> crt_limbs(const rs_ctx *ctx, int K) {
  using H = HostArith<M>;
  std::vector<CrtLimbT<M>> hl(ctx->L);  // value-initialised: zero, padding included
  for (int i = 0; i < ctx->L; i++) {
    const uint64_t t = ctx->q[i];
    hl[i].tmod = H::make(t);
    uint64_t Qm = 1 % t, F = 1 % t;
    for (int k = 0; k < K; k++) {
      hl[i].Qk_mod_t[k] = H::konst(ctx->Q[k] % t, t);
      Qm = host::mulmod(Qm, ctx->Q[k] % t, t);
    }
    for (int k = K; k < ctx->K; k++) F = host::mulmod(F, ctx->Q[k] % t, t);
    hl[i].Q_mod_t = H::plain(Qm, t);
    hl[i].F = H::konst(F, t);
    hl[i].scale = K < ctx->K;
  }
  return hl;
}

// decode_impl in the arithmetic M; the caller holds the context's WsScope
template <class M>
static int decode_arith(rs_ctx *ctx, int K, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings, int *h_budget,
                        bool guard, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  constexpr bool FP = std::is_same<M, Mod>::value;
  const int L = ctx->L, n = ctx->N_enc, logn = ctx->logN_enc;
  // Constants of the (context, level) that only decoding reads are built at the first call and kept on the device: the digits of
  // 2^b - 1 and the per-limb CRT constants.  With the table arrays of the context itself, a warm decode makes no
  // hipMalloc / hipFree and no pageable upload (each an implicit device-wide synchronisation; round-5 advice).
  if (!ctx->d_noise_thr[K]) {
    std::vector<uint64_t> digits;
    ctx->noise_tb[K] = noise_thresholds(ctx, K, digits);
    const std::vector<T> thr_h(digits.begin(), digits.end());  // plain values; digits < Q_k, and < 2^50 where T is double: exact
    ctx->d_noise_thr[K] = upload_constants(thr_h.data(), thr_h.size() * sizeof(T), "noise-threshold table");
  }
  if (!ctx->d_crt_limbs[K]) {
    const std::vector<CrtLimbT<M>> hl = crt_limbs<M>(ctx, K);
    ctx->d_crt_limbs[K] = upload_constants(hl.data(), hl.size() * sizeof(CrtLimbT<M>), "CRT constants");
  }
  const int tb = ctx->noise_tb[K];
  const T *d_thr = static_cast<const T *>(ctx->d_noise_thr[K]);
  const CrtLimbT<M> *d_limbs = static_cast<const CrtLimbT<M> *>(ctx->d_crt_limbs[K]);
  const CrtConstsT<M> cc = crt_consts<M>(ctx, K);
  int *d_bits = (int *)ws_get(ctx, WS_NOISE_BITS, sizeof(int) * count * (size_t)L);
  T *V = (T *)ws_get(ctx, WS_STAGE_ROWS, count * (size_t)L * K * n * sizeof(T));
  const size_t lds = padded_len((size_t)n) * sizeof(T);
  const int thr = enc_threads(logn);
  set_max_dyn_lds((const void *)decrypt_dot_kernel<M>, (int)lds);
  set_max_dyn_lds((const void *)crt_decode_kernel<M>, (int)lds);
  const double cts = (double)count * L, words = cts * K * n;  // ciphertexts; words of c0 (= of c1, = of V)
  {
    ProfScope p(ctx, st, CtxArith<M>::decrypt_dot_name, words * 8 * 3 + (double)K * n * 8,
                FP ? words * (7.0 + 7.0) + cts * K * ntt_fp64(n, logn) : 0.0);
    hipLaunchKernelGGL((decrypt_dot_kernel<M>), dim3((unsigned)(count * L), K), dim3(thr), lds, st, d_enc, d_sk, V, K, logn,
                       CtxArith<M>::d_coeff(ctx));
  }
  {
    ProfScope p(ctx, st, CtxArith<M>::crt_decode_name, words * 8 + (d_rings ? cts * ctx->N * 8 : 0.0) + cts * 4,
                FP ? cts * n * 7.0 * (K * (K - 1) / 2.0 + 2.0 * K) + (d_rings ? cts * ntt_fp64(n, logn) : 0.0) : 0.0);
    hipLaunchKernelGGL((crt_decode_kernel<M>), dim3((unsigned)(count * L)), dim3(thr), lds, st, V, d_rings, ctx->N, L, logn, cc, d_limbs,
                       ctx->d_index_map, CtxArith<M>::d_plain(ctx), d_thr, tb, d_bits);
  }
  RS_HIP(hipGetLastError());
  RS_HIP(hipStreamSynchronize(st));
  return noise_verdict(ctx, d_bits, count, tb, guard, h_budget);
}

int rs::decode_impl(rs_ctx *ctx, int K, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings, int *h_budget,
                    rs_stream stream) {
  if (count == 0) return RS_OK;
  WsScope ws_scope(ctx, S(stream));  // holds ctx->mu: the lazily built constants are built once
  int rc = RS_OK;
  dispatch_arith(ctx, [&](auto tag) { rc = decode_arith<decltype(tag)>(ctx, K, d_sk, d_enc, count, d_rings, h_budget, d_rings != nullptr, S(stream)); });
  return rc;
}

void rs::decode_held(rs_ctx *ctx, int K, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings, int *h_budget,
                     hipStream_t st) {
  if (count == 0) return;
  dispatch_arith(ctx, [&](auto tag) { decode_arith<decltype(tag)>(ctx, K, d_sk, d_enc, count, d_rings, h_budget, false, st); });
}

int rs::level_bit_count(const rs_ctx *ctx, int K) {
  BigU Q;
  Q.w[0] = 1;
  for (int k = 0; k < K; k++) Q.mul_add(ctx->Q[k], 0);
  return Q.bits();
}

extern "C" {

int rs_enc_encode(rs_ctx *ctx, const uint64_t *d_sk, const uint64_t *d_rings, size_t count, uint64_t seed, uint64_t *d_enc,
                  rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && d_sk && d_rings && d_enc, "null argument");
  if (count == 0) return RS_OK;
  RS_REQUIRE(ctx->N_enc <= 16 * 1024, "encoding degree out of range");
  WsScope ws_scope(ctx, S(stream));
  hipStream_t st = S(stream);
  const int thr = std::max(enc_threads(ctx->logN_enc), ctx->N_enc / 16);
  dispatch_arith(ctx, [&](auto tag) {
    using M = decltype(tag);
    const size_t lds = padded_len((size_t)ctx->N_enc) * sizeof(typename ArithOf<M>::T);
    set_max_dyn_lds((const void *)encode_kernel<M>, (int)lds);
    hipLaunchKernelGGL((encode_kernel<M>), dim3((unsigned)(count * ctx->L), ctx->K), dim3(thr), lds, st, d_rings, d_sk, d_enc, seed, ctx->N,
                       ctx->L, ctx->K, ctx->logN_enc, ctx->d_index_map, CtxArith<M>::d_plain(ctx), CtxArith<M>::d_coeff(ctx));
  });
  RS_HIP(hipGetLastError());
  RS_HIP(hipStreamSynchronize(st));
  RS_API_END
}

}  // extern "C"

// ---- wire format -----------------------------------------------------------------
// The reference declares serialisation of keys and proofs but never implements it
// (r1cs_ppzksnark.hpp:43-47,142-146; variable.tcc:391-414 throws).  Format (little endian):
//   u8[8]  magic "RSNKENC1"
//   u32    N, L, N_enc, K
//   u64    q[L], Q[K]
//   u64    count                       number of encoding elements
//   u8     empty[count]                1 = EMPTY element (seal_ring.tcc:412,432), payload all zero
//   pad to a multiple of 8 bytes
//   u64    payload[count][L][2][K][N_enc]   canonical residues, the layout of the ABI
// A stream of level K (modswitch.h) has K and Q[:K] in its header and K rows per component: exactly what a context
// created on the truncated prime list writes.  The functions below take the level; the context's own is ctx->K.
namespace rs {
static const char kMagic[8] = {'R', 'S', 'N', 'K', 'E', 'N', 'C', '1'};
static size_t wire_fixed_bytes(const rs_ctx *ctx, int K) { return 24 + 8 * (size_t)(ctx->L + K) + 8; }
static size_t wire_header_bytes(const rs_ctx *ctx, int K, size_t count) {
  const size_t raw = wire_fixed_bytes(ctx, K) + count;
  return (raw + 7) & ~(size_t)7;
}
static size_t level_enc_words(const rs_ctx *ctx, int K) { return (size_t)ctx->L * 2 * K * ctx->N_enc; }

size_t wire_size(const rs_ctx *ctx, int K, size_t count) {
  return wire_header_bytes(ctx, K, count) + count * level_enc_words(ctx, K) * sizeof(uint64_t);
}

void serialize_run(rs_ctx *ctx, int K, const uint64_t *d_enc, const uint8_t *h_empty, size_t count, void *h_buf, size_t buf_bytes,
                   hipStream_t st) {
  RS_REQUIRE(ctx && h_buf && (d_enc || count == 0), "null argument");
  RS_REQUIRE(buf_bytes >= wire_size(ctx, K, count), "buffer too small (rs_enc_wire_size)");
  uint8_t *p = (uint8_t *)h_buf;
  const size_t hb = wire_header_bytes(ctx, K, count), enc_bytes = level_enc_words(ctx, K) * sizeof(uint64_t);
  memset(p, 0, hb);
  memcpy(p, kMagic, 8);
  const uint32_t dims[4] = {(uint32_t)ctx->N, (uint32_t)ctx->L, (uint32_t)ctx->N_enc, (uint32_t)K};
  memcpy(p + 8, dims, 16);
  memcpy(p + 24, ctx->q, 8 * (size_t)ctx->L);
  memcpy(p + 24 + 8 * (size_t)ctx->L, ctx->Q, 8 * (size_t)K);
  const uint64_t c64 = count;
  uint8_t *q = p + 24 + 8 * (size_t)(ctx->L + K);
  memcpy(q, &c64, 8);
  for (size_t i = 0; i < count; i++) q[8 + i] = h_empty ? (h_empty[i] ? 1 : 0) : 0;
  if (count) {
    RS_HIP(hipMemcpyAsync(p + hb, d_enc, count * enc_bytes, hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    if (h_empty)
      for (size_t i = 0; i < count; i++)
        if (h_empty[i]) memset(p + hb + i * enc_bytes, 0, enc_bytes);
  }
}

// K_want: the level the stream must have, or 0: any 1 <= K <= ctx->K, reported in *K_found
void deserialize_run(rs_ctx *ctx, int K_want, const void *h_buf, size_t buf_bytes, uint64_t *d_enc, uint8_t *h_empty, size_t capacity,
                     size_t *h_count, int *K_found, hipStream_t st) {
  RS_REQUIRE(ctx && h_buf && h_count, "null argument");
  const uint8_t *p = (const uint8_t *)h_buf;
  RS_REQUIRE(buf_bytes >= (K_want ? wire_fixed_bytes(ctx, K_want) : 24), "truncated header");
  RS_REQUIRE(memcmp(p, kMagic, 8) == 0, "bad magic: not a ringsnark_amd encoding stream");
  uint32_t dims[4];
  memcpy(dims, p + 8, 16);
  RS_REQUIRE((int)dims[0] == ctx->N && (int)dims[1] == ctx->L && (int)dims[2] == ctx->N_enc &&
                 (K_want ? dims[3] == (uint32_t)K_want : dims[3] >= 1 && dims[3] <= (uint32_t)ctx->K),
             "stream was written for different ring / encoding dimensions");
  const int K = (int)dims[3];
  const size_t fixed = wire_fixed_bytes(ctx, K);
  RS_REQUIRE(buf_bytes >= fixed, "truncated header");
  RS_REQUIRE(memcmp(p + 24, ctx->q, 8 * (size_t)ctx->L) == 0 && memcmp(p + 24 + 8 * (size_t)ctx->L, ctx->Q, 8 * (size_t)K) == 0,
             "stream was written for different moduli");
  uint64_t c64;
  memcpy(&c64, p + 24 + 8 * (size_t)(ctx->L + K), 8);
  // The count is untrusted: bound it by what the buffer can hold BEFORE any size arithmetic (every
  // element costs one flag byte + enc_bytes of payload), so that nothing below can wrap.
  const size_t per = level_enc_words(ctx, K), enc_bytes = per * sizeof(uint64_t);
  RS_REQUIRE(c64 <= (uint64_t)((buf_bytes - fixed) / (1 + enc_bytes)), "truncated payload");
  const size_t count = (size_t)c64;
  RS_REQUIRE(buf_bytes >= wire_size(ctx, K, count), "truncated payload");
  const uint8_t *em = p + fixed;
  const size_t hb = wire_header_bytes(ctx, K, count);
  for (size_t i = 0; i < count; i++) RS_REQUIRE(em[i] <= 1, "corrupt empty flag");
  for (size_t i = fixed + count; i < hb; i++) RS_REQUIRE(p[i] == 0, "non-zero header padding");
  if (!d_enc) {  // size query (header validated)
    *h_count = count;
    if (K_found) *K_found = K;
    return;
  }
  RS_REQUIRE(capacity >= count, "destination holds fewer elements than the stream");
  const uint64_t *payload = (const uint64_t *)(p + hb);
  // canonical-residue check on the host: a proof from the wire is untrusted input
  const size_t n = (size_t)ctx->N_enc;
  for (size_t i = 0; i < count; i++)
    for (int l = 0; l < ctx->L; l++)
      for (int c = 0; c < 2; c++)
        for (int j = 0; j < K; j++) {
          const uint64_t *row = payload + i * per + (((size_t)l * 2 + c) * K + j) * n;
          const uint64_t Qj = ctx->Q[j];
          if (em[i]) {  // EMPTY element (seal_ring.tcc:412,432): the payload must be all zero
            for (size_t x = 0; x < n; x++) RS_REQUIRE(row[x] == 0, "non-zero payload of an EMPTY element");
          } else {
            for (size_t x = 0; x < n; x++) RS_REQUIRE(row[x] < Qj, "residue out of range");
          }
        }
  if (count) {
    RS_HIP(hipMemcpyAsync(d_enc, payload, count * per * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    RS_HIP(hipStreamSynchronize(st));
  }
  // outputs are written only after every check has passed
  if (h_empty) memcpy(h_empty, em, count);
  *h_count = count;
  if (K_found) *K_found = K;
}
}  // namespace rs

extern "C" {

size_t rs_enc_wire_size(const rs_ctx *ctx, size_t count) {
  if (!ctx) return 0;
  return wire_size(ctx, ctx->K, count);
}

int rs_enc_serialize(rs_ctx *ctx, const uint64_t *d_enc, const uint8_t *h_empty, size_t count, void *h_buf, size_t buf_bytes,
                     rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  serialize_run(ctx, ctx->K, d_enc, h_empty, count, h_buf, buf_bytes, S(stream));
  RS_API_END
}

int rs_enc_deserialize(rs_ctx *ctx, const void *h_buf, size_t buf_bytes, uint64_t *d_enc, uint8_t *h_empty, size_t capacity,
                       size_t *h_count, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  deserialize_run(ctx, ctx->K, h_buf, buf_bytes, d_enc, h_empty, capacity, h_count, nullptr, S(stream));
  RS_API_END
}

}  // extern "C"

// ---- r1cs_to_qrp_instance_map_with_evaluation --------------------------------------
// ringsnark/reductions/r1cs_to_qrp/r1cs_to_qrp.tcc:76-116 with util/evaluation_domain.tcc:21-50.
// What generator and verifier run before anything else (groth16.tcc:7-9, 127-128; rinocchio.tcc:7-9,
// 219-220).  The reference spends O(m^2) ring multiplications on the Lagrange polynomials; here
//     u_j(s) = Z(s) * (s - j)^-1 * c_j,   c_j = 1 / prod_{i != j} (j - i) = (-1)^(m-1-j) / (j! (m-1-j)!)
// (slot-constant c_j), one batched ring inversion, and At / Bt / Ct = transpose(A/B/C) * u through
// the same sparse kernel as row a14 on the transposed CSR.  Every value is a canonical residue of an
// exact ring expression, hence bit-identical to the reference's order of operations.
namespace rs {
// Per slot, with d_j = s - j:  Ht[j] = s^j (j <= m),  Zt = prod_j d_j,  and the Lagrange values
//     u_j = c_j * prod_{i != j} d_i = c_j * (prod_{i < j} d_i) * (prod_{i > j} d_i)
// by a backward pass (suffix products parked in U) and a forward pass (running prefix): no
// division, so a slot in which s happens to equal a domain element is handled exactly like the
// reference's product loop (evaluation_domain.tcc:28-39).  hit[0] / hit[1] = min / max over slots of
// the domain index the slot equals (0xFFFFFFFF: none): s IS a domain element -- the only case the
// reference rejects (evaluation_domain.tcc:24-26) -- iff hit[0] == hit[1] != 0xFFFFFFFF.
template <class M>
__global__ void __launch_bounds__(256)
lagrange_kernel(const uint64_t *__restrict__ s, uint64_t *__restrict__ Ht, uint64_t *__restrict__ U, uint64_t *__restrict__ Zt,
                const typename ArithOf<M>::T *__restrict__ c /* [L][m], table constants */, unsigned *__restrict__ hit, size_t m, int N, int L,
                const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t S = (size_t)L * N, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const int limb = (int)(i / (size_t)N);
  const M mod = qmod[limb];
  const T sv = center(from_res<T>(s[i]), mod);
  unsigned my_hit = 0xFFFFFFFFu;
  T suf = T(1);
  for (size_t j = m; j-- > 0;) {
    U[j * S + i] = to_res(canon(suf, mod));
    const T d = reduce(subm(sv, small_val((uint64_t)j, mod), mod), mod);
    if (canon(d, mod) == T(0)) my_hit = (unsigned)j;
    suf = mulmod_dd(suf, d, mod);
  }
  Zt[i] = to_res(canon(suf, mod));
  T pre = T(1), pw = T(1);
  for (size_t j = 0; j <= m; j++) {
    Ht[j * S + i] = to_res(canon(pw, mod));
    pw = mulmod_dd(pw, sv, mod);
    if (j < m) {
      const T v = mulmod_dd(pre, center(from_res<T>(U[j * S + i]), mod), mod);
      U[j * S + i] = to_res(canon(mulmod(v, c[(size_t)limb * m + j], mod), mod));
      pre = mulmod_dd(pre, reduce(subm(sv, small_val((uint64_t)j, mod), mod), mod), mod);
    }
  }
  atomicMin(&hit[0], my_hit);
  atomicMax(&hit[1], my_hit);
}
}  // namespace rs

namespace rs {
void instance_map_run(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *d_At, uint64_t *d_Bt, uint64_t *d_Ct,
                      uint64_t *d_Ht, uint64_t *d_Zt, hipStream_t st, bool wipe) {
  const size_t m = cs->m, SW = ctx->ring_words();
  const int L = ctx->L;
  uint64_t *D = nullptr;
  RS_HIP(hipMalloc(&D, m * SW * sizeof(uint64_t)));
  struct Guard {
    std::vector<void *> p;
    rs_r1cs *tr = nullptr;
    void *wipe_p = nullptr;  // overwritten with zeros before the release (nothing enqueued may still use it: the stream is drained first)
    size_t wipe_bytes = 0;
    hipStream_t st = nullptr;
    ~Guard() {
      if (wipe_p) {
        (void)hipStreamSynchronize(st);
        (void)hipMemset(wipe_p, 0, wipe_bytes);
        (void)hipDeviceSynchronize();
      }
      for (void *x : p) (void)hipFree(x);
      if (tr) rs_r1cs_destroy(tr);
    }
  } guard;
  guard.p.push_back(D);
  guard.st = st;
  if (wipe) guard.wipe_p = D, guard.wipe_bytes = m * SW * sizeof(uint64_t);
  std::vector<uint64_t> hc;  // slot-constant factors c_j [L][m], table constants of the context's arithmetic as 64-bit words
  dispatch_arith(ctx, [&](auto tag) { lagrange_constants<decltype(tag)>(ctx, m, hc); });
  uint64_t *d_c = nullptr;
  RS_HIP(hipMalloc(&d_c, hc.size() * sizeof(uint64_t)));
  guard.p.push_back(d_c);
  unsigned *d_hit = nullptr;
  RS_HIP(hipMalloc(&d_hit, 2 * sizeof(unsigned)));
  guard.p.push_back(d_hit);
  const unsigned hit0[2] = {0xFFFFFFFFu, 0u};
  unsigned hit[2];
  RS_HIP(hipMemcpyAsync(d_c, hc.data(), hc.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  RS_HIP(hipMemcpyAsync(d_hit, hit0, sizeof(hit0), hipMemcpyHostToDevice, st));
  dispatch_arith(ctx, [&](auto tag) {
    using M = decltype(tag);
    hipLaunchKernelGGL((lagrange_kernel<M>), dim3((unsigned)((SW + 255) / 256)), dim3(256), 0, st, d_s, d_Ht, D, d_Zt,
                       reinterpret_cast<const typename ArithOf<M>::T *>(d_c), d_hit, m, ctx->N, L, CtxArith<M>::qmod(ctx));
  });
  RS_HIP(hipGetLastError());
  RS_HIP(hipMemcpyAsync(hit, d_hit, sizeof(hit), hipMemcpyDeviceToHost, st));
  RS_HIP(hipStreamSynchronize(st));  // hc, hit
  // evaluation_domain.tcc:24-26: rejected only when s equals a domain element AS A RING ELEMENT
  // (every slot of every limb equal to the same j)
  if (hit[0] == hit[1] && hit[0] != 0xFFFFFFFFu)
    throw Error(RS_ERR_NOT_INVERTIBLE, "t cannot be one of the values in the domain");
  // transposed system: row k (variable k, 0 = the constant one) holds (constraint i + 1, coeff)
  const size_t rows = cs->n_vars + 1;
  std::vector<uint32_t> rp[3], col[3];
  std::vector<uint64_t> cf[3];
  std::vector<int32_t> pi[3];  // polynomial coefficients travel with their terms (same table)
  const uint32_t *rpp[3], *colp[3];
  const uint64_t *cfp[3];
  const int32_t *pip[3];
  size_t nnz[3];
  for (int w = 0; w < 3; w++) {
    const size_t z = cs->nnz[w];
    nnz[w] = z;
    rp[w].assign(rows + 1, 0);
    for (size_t e = 0; e < z; e++) rp[w][cs->h_col[w][e] + 1]++;
    for (size_t k = 0; k < rows; k++) rp[w][k + 1] += rp[w][k];
    col[w].resize(std::max<size_t>(z, 1));
    cf[w].resize(std::max<size_t>((size_t)L * z, 1));
    pi[w].assign(std::max<size_t>(z, 1), -1);
    std::vector<uint32_t> fill(rp[w].begin(), rp[w].end() - 1);
    for (size_t i = 0; i < m; i++)
      for (uint32_t e = cs->h_row_ptr[w][i]; e < cs->h_row_ptr[w][i + 1]; e++) {
        const uint32_t dst = fill[cs->h_col[w][e]]++;
        col[w][dst] = (uint32_t)(i + 1);
        for (int l = 0; l < L; l++) cf[w][(size_t)l * z + dst] = cs->h_coeff[w][(size_t)l * z + e];
        if (!cs->h_pidx[w].empty()) pi[w][dst] = cs->h_pidx[w][e];
      }
    rpp[w] = rp[w].data();
    colp[w] = col[w].data();
    cfp[w] = cf[w].data();
    pip[w] = cs->h_pidx[w].empty() ? nullptr : pi[w].data();
  }
  RS_REQUIRE(rs_r1cs_create_poly(ctx, rows, m, 0, rpp, colp, cfp, nnz, pip, cs->n_poly ? cs->h_ptab.data() : nullptr, cs->n_poly,
                                 &guard.tr) == RS_OK,
             rs_last_error());
  uint64_t *outs[3] = {d_At, d_Bt, d_Ct};
  for (int w = 0; w < 3; w++) r1cs_evaluate_run(ctx, guard.tr, w, RS_EVAL_FULL, D, outs[w], st);
  RS_HIP(hipGetLastError());
  RS_HIP(hipStreamSynchronize(st));
}
}  // namespace rs

extern "C" {

int rs_instance_map_eval(rs_ctx *ctx, const rs_r1cs *cs, const uint64_t *d_s, uint64_t *d_At, uint64_t *d_Bt, uint64_t *d_Ct,
                         uint64_t *d_Ht, uint64_t *d_Zt, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(ctx && cs && d_s && d_At && d_Bt && d_Ct && d_Ht && d_Zt, "null argument");
  instance_map_run(ctx, cs, d_s, d_At, d_Bt, d_Ct, d_Ht, d_Zt, S(stream), false);
  RS_API_END
}

}  // extern "C"
