// modswitch.hip -- EncodingElem::modswitch_inplace (ringsnark/seal/seal_ring.hpp:370, seal_ring.tcc:317-322) on the device
// and the entry points that read an encoding of fewer primes (include/ringsnark_amd/modswitch.h).
//
// One step K_in -> K_in - 1 is SEAL 4.x BGV mod_t_and_divide_q_last_ntt_inplace (un-vendored dependency; its published
// algorithm) per (element, limb i, component c), t = q_i, p = Q[K_in - 1]:
//     last = iNTT_p(row K_in - 1)                 canonical in [0, p)
//     u    = (-last * p^-1) mod t                 canonical in [0, t)
//     c'_j = (c_j - NTT_{Q_j}((last + u p) mod Q_j)) * p^-1 mod Q_j        for every j < K_in - 1
// last + u p = 0 mod p and = last mod t, so subtracting it makes the ciphertext divisible by p without moving the
// plaintext; the division leaves m * p^-1 mod t, which the level decode undoes (encoding.hip, CrtLimbT::F).
// Every quantity is a residue: whichever representatives the arithmetic holds on the way, the words written are the
// canonical ones, so the kernel's output is defined by the three lines above alone (ringsnark_amd/modswitch.py).
//
// Work shape: one workgroup per (element, limb, component, target prime j).  A proof is 3..9 elements of 2 L polynomials,
// so the K_in - 1 target rows of a polynomial are what fills the device; each workgroup repeats the inverse transform of the
// dropped row.  One workgroup per polynomial, the dropped row's coefficients kept in registers across its K_in - 1 targets,
// took 1.6 to 1.9 times as long at the C3 shape (DESIGN.md "Mod-switched proofs", profiles/modswitch.txt).
#include <algorithm>
#include <cstring>

#include "../../include/ringsnark_amd/modswitch.h"
#include "ntt_core.hpp"
#include "rs_internal.hpp"

namespace rs {

// constants of one step (dropping p) in the context's arithmetic: table constants, i.e. multipliers
template <class M>
struct SwitchConsts {
  typename ArithOf<M>::T pinv_t[RS_MAX_L];  // p^-1 mod q_i
  typename ArithOf<M>::T p_mod_Q[RS_MAX_K];  // p mod Q_j
  typename ArithOf<M>::T pinv_Q[RS_MAX_K];   // p^-1 mod Q_j
};

// a canonical residue of one prime as a multiplication operand of another
__device__ __forceinline__ double rebase(double v, const Mod &m) { return reduce(v, m); }
__device__ __forceinline__ uint64_t rebase(uint64_t v, const ModI &m) { return v % m.p; }

// grid (count * L * 2, K_in - 1): blockIdx.x = (element * L + limb) * 2 + component, blockIdx.y = the target row j.
// in [.][K_in][n], out [.][K_in - 1][n].  Outside the transforms a thread touches only the positions threadIdx.x + k * blockDim.x
// of the LDS tile, before and after: no barrier is needed between the scaling of `last` and the correction term.
template <class M>
__global__ void __launch_bounds__(1024)
mod_switch_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, int K_in, int L, int logn, SwitchConsts<M> sc,
                  const NttTableT<typename ArithOf<M>::T, M> *__restrict__ coeff_tabs, const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T *s = reinterpret_cast<T *>(smem);
  const int n = 1 << logn, j = blockIdx.y;
  const size_t poly = blockIdx.x;
  const int limb = (int)((poly >> 1) % (size_t)L);
  const M tmod = qmod[limb];
  const NttTableT<T, M> ptab = coeff_tabs[K_in - 1], tab = coeff_tabs[j];
  const M pmod = ptab.mod, mod = tab.mod;
  const uint64_t *src = in + poly * (size_t)K_in * n;
  const uint64_t *dropped = src + (size_t)(K_in - 1) * n, *cj = src + (size_t)j * n;
  uint64_t *oj = out + (poly * (size_t)(K_in - 1) + j) * n;
  for (int x = threadIdx.x; x < n; x += blockDim.x) s[pidx(x)] = from_res<T>(dropped[x]);
  __syncthreads();
  lds_ntt_inv(s, logn, ptab.d_itw, 1, pmod, ptab.inv_red_mask);
  for (int x = threadIdx.x; x < n; x += blockDim.x) {
    const T last = canon(mulmod(reduce(s[pidx(x)], pmod), ptab.ninv, pmod), pmod);  // in [0, p)
    const T u = canon(negm(mulmod(rebase(last, tmod), sc.pinv_t[limb], tmod), tmod), tmod);  // in [0, t)
    s[pidx(x)] = reduce(addm(rebase(last, mod), mulmod(rebase(u, mod), sc.p_mod_Q[j], mod), mod), mod);
  }
  __syncthreads();
  lds_ntt_fwd(s, logn, tab.d_tw, 1, mod, tab.fwd_red_mask);
  for (int x = threadIdx.x; x < n; x += blockDim.x) {
    const T d = reduce(subm(from_res<T>(cj[x]), reduce(s[pidx(x)], mod), mod), mod);
    oj[x] = to_res(canon(mulmod(d, sc.pinv_Q[j], mod), mod));
  }
}

// one step: src [polys][K_in][n] -> dst [polys][K_in - 1][n]
template <class M>
static void mod_switch_step(rs_ctx *ctx, const uint64_t *src, uint64_t *dst, size_t polys, int K_in, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const uint64_t p = ctx->Q[K_in - 1];
  SwitchConsts<M> sc;
  memset(&sc, 0, sizeof(sc));
  for (int i = 0; i < ctx->L; i++) sc.pinv_t[i] = HostArith<M>::konst(host::invmod(p % ctx->q[i], ctx->q[i]), ctx->q[i]);
  for (int j = 0; j < K_in - 1; j++) {
    sc.p_mod_Q[j] = HostArith<M>::konst(p % ctx->Q[j], ctx->Q[j]);
    sc.pinv_Q[j] = HostArith<M>::konst(host::invmod(p % ctx->Q[j], ctx->Q[j]), ctx->Q[j]);
  }
  const int n = ctx->N_enc, logn = ctx->logN_enc;
  const size_t lds = padded_len((size_t)n) * sizeof(T);
  set_max_dyn_lds((const void *)mod_switch_kernel<M>, (int)lds);
  const double words = (double)polys * n;
  {
    // algorithmic bytes: every input row once, every output row once; per output row one inverse and one forward transform
    ProfScope prof(ctx, st, "mod_switch_kernel", words * 8 * (2.0 * K_in - 1),
                   ctx->use_int ? 0.0 : (K_in - 1) * ((double)polys * 2 * ntt_fp64(n, logn) + words * 7.0 * 5));
    hipLaunchKernelGGL(mod_switch_kernel<M>, dim3((unsigned)polys, (unsigned)(K_in - 1)), dim3(enc_threads(logn)), lds, st, src, dst, K_in,
                       ctx->L, logn, sc, CtxArith<M>::d_coeff(ctx), CtxArith<M>::qmod(ctx));
  }
  RS_HIP(hipGetLastError());
}

static size_t level_words(const rs_ctx *ctx, int K, size_t count) { return count * (size_t)ctx->L * 2 * K * ctx->N_enc; }

static void mod_switch_run(rs_ctx *ctx, const uint64_t *d_in, size_t count, int K_in, int K_out, uint64_t *d_out, hipStream_t st) {
  RS_REQUIRE(K_out >= 1 && K_out <= K_in && K_in <= ctx->K, "levels out of range: 1 <= K_out <= K_in <= K");
  if (count == 0) return;
  RS_REQUIRE(d_in && d_out, "null argument");
  const size_t polys = count * (size_t)ctx->L * 2;
  RS_REQUIRE(polys < ((size_t)1 << 31), "too many elements in one call");
  const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + level_words(ctx, K_in, count) * sizeof(uint64_t);
  const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + level_words(ctx, K_out, count) * sizeof(uint64_t);
  RS_REQUIRE(a1 <= b0 || b1 <= a0, "input and output overlap: the switch is out of place");
  if (K_in == K_out) {
    RS_HIP(hipMemcpyAsync(d_out, d_in, a1 - a0, hipMemcpyDeviceToDevice, st));
    return;
  }
  WsScope ws_scope(ctx, st);
  uint64_t *level[2] = {nullptr, nullptr};  // the intermediate levels K_in - 1, K_in - 2, .. in turn
  if (K_in - K_out > 1) {
    const size_t w0 = level_words(ctx, K_in - 1, count), w1 = level_words(ctx, K_in - 2, count);
    level[0] = (uint64_t *)ws_get(ctx, WS_MODSWITCH_LEVELS, (w0 + w1) * sizeof(uint64_t));
    level[1] = level[0] + w0;
  }
  const uint64_t *src = d_in;
  for (int k = K_in, step = 0; k > K_out; k--, step++) {
    uint64_t *dst = k - 1 == K_out ? d_out : level[step & 1];
    dispatch_arith(ctx, [&](auto tag) { mod_switch_step<decltype(tag)>(ctx, src, dst, polys, k, st); });
    src = dst;
  }
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_enc_mod_switch(rs_ctx *ctx, const uint64_t *d_in, size_t count, int K_in, int K_out, uint64_t *d_out, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  mod_switch_run(ctx, d_in, count, K_in, K_out, d_out, S(stream));
  RS_API_END
}

int rs_enc_decode_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, uint64_t *d_rings,
                        rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(K_lvl >= 1 && K_lvl <= ctx->K, "level out of range: 1 <= K_lvl <= K");
  RS_REQUIRE(d_sk && d_enc && d_rings, "null argument");
  return decode_impl(ctx, K_lvl, d_sk, d_enc, count, d_rings, nullptr, stream);
  RS_API_END
}

int rs_enc_noise_budget_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_sk, const uint64_t *d_enc, size_t count, int *h_budget,
                              rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(K_lvl >= 1 && K_lvl <= ctx->K, "level out of range: 1 <= K_lvl <= K");
  RS_REQUIRE(d_sk && d_enc && h_budget, "null argument");
  return decode_impl(ctx, K_lvl, d_sk, d_enc, count, nullptr, h_budget, stream);
  RS_API_END
}

size_t rs_enc_wire_size_level(const rs_ctx *ctx, int K_lvl, size_t count) {
  if (!ctx || K_lvl < 1 || K_lvl > ctx->K) return 0;
  return wire_size(ctx, K_lvl, count);
}

int rs_enc_serialize_level(rs_ctx *ctx, int K_lvl, const uint64_t *d_enc, const uint8_t *h_empty, size_t count, void *h_buf,
                           size_t buf_bytes, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(K_lvl >= 1 && K_lvl <= ctx->K, "level out of range: 1 <= K_lvl <= K");
  serialize_run(ctx, K_lvl, d_enc, h_empty, count, h_buf, buf_bytes, S(stream));
  RS_API_END
}

int rs_enc_deserialize_level(rs_ctx *ctx, const void *h_buf, size_t buf_bytes, uint64_t *d_enc, uint8_t *h_empty, size_t capacity,
                             size_t *h_count, int *h_K_lvl, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(h_K_lvl != nullptr, "null argument");
  deserialize_run(ctx, 0, h_buf, buf_bytes, d_enc, h_empty, capacity, h_count, h_K_lvl, S(stream));
  RS_API_END
}

}  // extern "C"
