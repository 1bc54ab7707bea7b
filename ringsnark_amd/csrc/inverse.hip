// inverse.hip -- rs_ring_inv_or_zero (include/ringsnark_amd/inverse.h): the slotwise inverse-or-zero of ring elements, and
// with a numerator their slotwise quotients -- the wires of the is-zero gadget and of a division, which a constraint
// determines only through its a or b side.
//
// BATCHING.  A thread inverts a batch of n = 16 words with one Fermat power (Montgomery's trick): 3 (n - 1) = 45 products and
// one power of 52 (FP64) or 62 (Montgomery) squarings, about 8 products a word where ring_inv_kernel (rs_core.hip) spends
// about 78.  The batch is the thread's eight 16-byte words of a piece, kept as TWO chains of eight -- the .x words and the .y
// words -- that meet in one product before the power: the same 45 products, two independent dependency chains per lane.
// n = 16 does not spill on gfx950 (resource usage of the four instantiations: DESIGN.md, "Inverse-or-zero wires").
//
// NUMBERING OF THE WORK.  The limb is OUTERMOST, then (element, slot pair): a piece is 256 * 8 consecutive slot pairs of ONE
// limb (consecutive elements follow each other in this numbering), and the pieces of limb 0 come before those of limb 1.  So
// the words of a batch share one modulus at every N -- also at N = 32, where a limb row is 16 slot pairs and a piece holds
// 128 elements -- and that modulus is uniform over the workgroup: its constants are read through the scalar path, as
// ring_pointwise_kernel reads them for a piece inside a limb row.
//
// ACCESS SHAPE of bits.hip and ring_pointwise_kernel: 16-byte loads and stores, eight per operand in flight per lane before
// the first use, pieces dealt round-robin to a bounded grid, a guarded variant for the last piece of a limb, non-temporal
// stores once the output reaches 64 MiB.
//
// Every reported field is a function of the inputs only:
//   n_zero, n_bad     integer atomicAdd of per-workgroup counts
//   first zero / bad  64-bit atomicMin over the key element * L*N + limb * N + slot
//   bad_x, bad_num    two loads at the minimal bad key, by the second kernel
// Input with no zero and no bad word issues no atomic: a wave votes on one mask per piece and goes on.  A wave that saw one
// adds two 16-bit masks per lane to a tally in registers (no second pass over the input); the tallies are reduced ONCE, when
// the workgroup has done its last piece: one add per count and at most one min per key for a WORKGROUP, not for a wave and
// piece -- with half of the slots zero, atomics per wave and piece on two addresses took four times as long as the arithmetic
// (DESIGN.md).  The min is skipped where a plain read of the key already shows a smaller one (keys only ever decrease).
#include <cstdint>
#include <string>

#include "../../include/ringsnark_amd/inverse.h"
#include "inverse_batch.hpp"

namespace rs {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));  // as in ntt_wide.hpp

constexpr int INV_U = 8;                                  // 16-byte words of a thread's batch: n = 2 * INV_U words
constexpr size_t INV_PIECE = (size_t)256 * INV_U;         // slot pairs of a piece
// device side of the report: [0] key of the first zero (all ones: none), [1] key of the first bad position, [2] zeros,
// [3] bad positions, [4] the x word, [5] the num word there
constexpr int INV_WORDS = 6;
// InvTally, inv_enter, inv_fermat and inv_report: inverse_batch.hpp, shared with the solver's hint steps (r1cs_hints.hip)

struct InvArgs {
  size_t per_limb;       // count * P slot pairs of one limb
  size_t pieces_limb;    // pieces of one limb
  size_t xs, ns, os;     // x_stride, num_stride, out_stride in 16-byte words: stride * L * P
  int logP, L;           // P = N / 2 slot pairs per limb row
};

// One piece of limb `limb`.  GUARD: the last piece of a limb, which may end before its 2048th slot pair.
template <class M, bool HAS_NUM, bool NT, bool GUARD>
__device__ __forceinline__ void inv_piece(const u64x2 *__restrict__ x, const u64x2 *__restrict__ num, u64x2 *__restrict__ out, const InvArgs &a,
                                          int limb, size_t base, const M m, InvTally &tally) {
  using T = typename ArithOf<M>::T;
  const size_t P = (size_t)1 << a.logP, row = (size_t)limb * P;
  u64x2 v[INV_U], w[INV_U];
  size_t oo[INV_U];
  bool live[INV_U];
#pragma unroll
  for (int u = 0; u < INV_U; u++) {
    const size_t t = base + threadIdx.x + 256 * u;
    live[u] = !GUARD || t < a.per_limb;
    const size_t e = t >> a.logP, p = t & (P - 1);
    oo[u] = e * a.os + row + p;
    v[u] = u64x2{1ull, 1ull};  // a slot pair past the end: a factor 1, not a zero
    w[u] = u64x2{1ull, 1ull};
    if (live[u]) {
      v[u] = x[e * a.xs + row + p];
      if (HAS_NUM) w[u] = num[e * a.ns + row + p];
    }
  }
  // masks over the batch, bit 2u for .x and 2u + 1 for .y: bad words; words replaced by 1 (zero or bad)
  const uint64_t q = modulus_u64(m);
  unsigned bad = 0, gone = 0;
#pragma unroll
  for (int u = 0; u < INV_U; u++) {
    const bool b0 = v[u].x >= q || (HAS_NUM && w[u].x >= q), b1 = v[u].y >= q || (HAS_NUM && w[u].y >= q);
    const bool g0 = b0 || v[u].x == 0, g1 = b1 || v[u].y == 0;
    bad |= (b0 ? 1u : 0u) << (2 * u) | (b1 ? 2u : 0u) << (2 * u);
    gone |= (g0 ? 1u : 0u) << (2 * u) | (g1 ? 2u : 0u) << (2 * u);
    if (g0) v[u].x = 1ull;
    if (g1) v[u].y = 1ull;
  }
  // prefix products of the two chains, one power of their product, back-substitution
  T fx[INV_U], fy[INV_U], px[INV_U], py[INV_U];
#pragma unroll
  for (int u = 0; u < INV_U; u++) {
    fx[u] = inv_enter<M>(v[u].x, m);
    fy[u] = inv_enter<M>(v[u].y, m);
  }
  px[0] = fx[0];
  py[0] = fy[0];
#pragma unroll
  for (int u = 1; u < INV_U; u++) {
    px[u] = mulmod(px[u - 1], fx[u], m);
    py[u] = mulmod(py[u - 1], fy[u], m);
  }
  const T one = inv_enter<M>(1ull, m);
  const T all = inv_fermat<M>(mulmod(px[INV_U - 1], py[INV_U - 1], m), one, m);
  T ix = mulmod(all, py[INV_U - 1], m), iy = mulmod(all, px[INV_U - 1], m);  // the inverses of the chains' totals
#pragma unroll
  for (int u = INV_U - 1; u >= 0; u--) {
    T rx = ix, ry = iy;  // u == 0: what is left is the inverse of the first word
    if (u > 0) {
      rx = mulmod(ix, px[u - 1], m);
      ry = mulmod(iy, py[u - 1], m);
      ix = mulmod(ix, fx[u], m);
      iy = mulmod(iy, fy[u], m);
    }
    // out of the domain: times the numerator as a data word, or times 1 (konst_value)
    u64x2 o;
    if (HAS_NUM) {
      const uint64_t n0 = (bad >> (2 * u)) & 1u ? 0ull : w[u].x, n1 = (bad >> (2 * u + 1)) & 1u ? 0ull : w[u].y;
      o.x = to_res(canon(mulmod(center(from_res<T>(n0), m), rx, m), m));
      o.y = to_res(canon(mulmod(center(from_res<T>(n1), m), ry, m), m));
    } else {
      o.x = to_res(canon(konst_value(rx, m), m));
      o.y = to_res(canon(konst_value(ry, m), m));
    }
    if ((gone >> (2 * u)) & 1u) o.x = 0ull;
    if ((gone >> (2 * u + 1)) & 1u) o.y = 0ull;
    if (!live[u]) continue;
    if (NT) __builtin_nontemporal_store(o, out + oo[u]);
    else out[oo[u]] = o;
  }
  if (__ballot(gone != 0u) == 0ull) return;  // wave-uniform: the common path ends here
  // inside a lane the keys ascend with the bit index
  const unsigned zero = gone & ~bad;
  const size_t S = 2 * P * (size_t)a.L;
  tally.nz += __popc(zero);
  tally.nb += __popc(bad);
  if (zero) {
    const int j = __ffs(zero) - 1;
    const size_t t = base + threadIdx.x + 256 * (size_t)(j >> 1);
    const unsigned long long k = (t >> a.logP) * S + 2 * (row + (t & (P - 1))) + (size_t)(j & 1);
    tally.kz = k < tally.kz ? k : tally.kz;
  }
  if (bad) {
    const int j = __ffs(bad) - 1;
    const size_t t = base + threadIdx.x + 256 * (size_t)(j >> 1);
    const unsigned long long k = (t >> a.logP) * S + 2 * (row + (t & (P - 1))) + (size_t)(j & 1);
    tally.kb = k < tally.kb ? k : tally.kb;
  }
}

// NT: non-temporal stores (outputs larger than the caches they would otherwise sweep, written once)
template <class M, bool HAS_NUM, bool NT>
__global__ void __launch_bounds__(256) ring_inv_or_zero_kernel(const u64x2 *__restrict__ x, const u64x2 *__restrict__ num, u64x2 *__restrict__ out,
                                                               InvArgs a, const M *__restrict__ qmod, unsigned long long *__restrict__ rep) {
  const size_t pieces = a.pieces_limb * (size_t)a.L;
  InvTally tally;
  for (size_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
    const int limb = (int)(piece / a.pieces_limb);  // uniform over the workgroup: qmod[limb] is a scalar load
    const size_t base = (piece - (size_t)limb * a.pieces_limb) * INV_PIECE;
    const M m = qmod[limb];
    if (base + INV_PIECE <= a.per_limb) inv_piece<M, HAS_NUM, NT, false>(x, num, out, a, limb, base, m, tally);
    else inv_piece<M, HAS_NUM, NT, true>(x, num, out, a, limb, base, m, tally);
  }
  inv_report(tally, rep);
}

// the two words at the first bad position
__global__ void ring_inv_or_zero_finish_kernel(const u64x2 *__restrict__ x, const u64x2 *__restrict__ num, InvArgs a, unsigned long long *__restrict__ rep) {
  const unsigned long long key = rep[1];  // final: written by the launch before this one
  if (threadIdx.x != 0 || key == ~0ull) return;
  const size_t P = (size_t)1 << a.logP, S = 2 * P * (size_t)a.L;
  const size_t e = (size_t)(key / S), idx = (size_t)(key % S);
  rep[4] = reinterpret_cast<const unsigned long long *>(x + e * a.xs)[idx];
  rep[5] = num ? reinterpret_cast<const unsigned long long *>(num + e * a.ns)[idx] : 0ull;
}

// a * b, or RS_ERR_INVALID when the product does not fit
static size_t inv_mul_fit(size_t a, size_t b) {
  size_t r = 0;
  RS_REQUIRE(!__builtin_mul_overflow(a, b, &r) && r < ((size_t)1 << 60), "count, strides and ring size address more than 2^60 words");
  return r;
}

// No row of `in` (count rows of `words` words, in_words apart) may share a word with a row of out: both are ascending runs
// of disjoint intervals (strides >= 1), so one merge over the two decides it exactly (as in bits.hip).
static void inv_require_disjoint(const char *what, uintptr_t in0, size_t in_words, uintptr_t out0, size_t out_words, size_t count, size_t words) {
  const size_t in_extent = inv_mul_fit(count - 1, in_words) + words, out_extent = inv_mul_fit(count - 1, out_words) + words;
  RS_REQUIRE(in0 + 8 * in_extent > in0 && out0 + 8 * out_extent > out0, "count, strides and ring size address more than 2^60 words");
  if (in0 + 8 * in_extent <= out0 || out0 + 8 * out_extent <= in0) return;
  for (size_t i = 0, j = 0; i < count && j < count;) {
    const uintptr_t xi = in0 + 8 * i * in_words, oj = out0 + 8 * j * out_words;
    if (xi + 8 * words <= oj) i++;
    else if (oj + 8 * words <= xi) j++;
    else
      throw Error(RS_ERR_INVALID, std::string(what) + " element " + std::to_string(i) + " shares a word with output element " + std::to_string(j) +
                                      ": no input row may overlap an output row");
  }
}

template <class M, bool HAS_NUM>
static void inv_launch(rs_ctx *ctx, const u64x2 *x, const u64x2 *num, u64x2 *out, const InvArgs &a, bool nt, unsigned blocks, unsigned long long *rep,
                       hipStream_t st) {
  if (nt)
    hipLaunchKernelGGL((ring_inv_or_zero_kernel<M, HAS_NUM, true>), dim3(blocks), dim3(256), 0, st, x, num, out, a, CtxArith<M>::qmod(ctx), rep);
  else
    hipLaunchKernelGGL((ring_inv_or_zero_kernel<M, HAS_NUM, false>), dim3(blocks), dim3(256), 0, st, x, num, out, a, CtxArith<M>::qmod(ctx), rep);
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_ring_inv_or_zero(rs_ctx *ctx, const uint64_t *d_x, size_t x_stride, const uint64_t *d_num, size_t num_stride, size_t count,
                        uint64_t *d_out, size_t out_stride, rs_inv_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  rs_inv_report r{};
  if (count == 0) {
    if (h_report) *h_report = r;
    return RS_OK;
  }
  RS_REQUIRE(d_x && d_out, "null argument");
  RS_REQUIRE(x_stride >= 1, "x_stride must be at least 1 ring element");
  RS_REQUIRE(out_stride >= 1, "out_stride must be at least 1 ring element");
  RS_REQUIRE(!d_num || num_stride >= 1, "num_stride must be at least 1 ring element");
  int logN = 0;
  while ((1 << logN) < ctx->N) logN++;
  RS_REQUIRE((1 << logN) == ctx->N && logN >= 1, "ring degree must be a power of two, at least 2");
  RS_REQUIRE((((uintptr_t)d_x | (uintptr_t)d_num | (uintptr_t)d_out) & 15u) == 0, "d_x, d_num and d_out must be 16-byte aligned");
  const size_t words = ctx->ring_words(), P = (size_t)ctx->N / 2;
  const size_t xs_words = inv_mul_fit(x_stride, words), os_words = inv_mul_fit(out_stride, words);
  const size_t ns_words = d_num ? inv_mul_fit(num_stride, words) : 0;
  inv_require_disjoint("x", (uintptr_t)d_x, xs_words, (uintptr_t)d_out, os_words, count, words);
  if (d_num) inv_require_disjoint("num", (uintptr_t)d_num, ns_words, (uintptr_t)d_out, os_words, count, words);
  InvArgs a{};
  a.per_limb = inv_mul_fit(count, P);
  a.pieces_limb = (a.per_limb + INV_PIECE - 1) / INV_PIECE;
  a.xs = xs_words / 2;
  a.ns = ns_words / 2;
  a.os = os_words / 2;
  a.logP = logN - 1;
  a.L = ctx->L;
  const u64x2 *x = reinterpret_cast<const u64x2 *>(d_x), *num = reinterpret_cast<const u64x2 *>(d_num);
  u64x2 *out = reinterpret_cast<u64x2 *>(d_out);
  const unsigned blocks = (unsigned)std::min<size_t>(a.pieces_limb * (size_t)ctx->L, 256 * 8);  // a bounded grid: the workgroups stride over the pieces
  hipStream_t st = S(stream);
  WsScope ws_scope(ctx, st);
  unsigned long long *rep = (unsigned long long *)ws_get(ctx, WS_SMALL, 256);
  RS_HIP(hipMemsetAsync(rep, 0, sizeof(unsigned long long) * INV_WORDS, st));
  RS_HIP(hipMemsetAsync(rep, 0xFF, sizeof(unsigned long long) * 2, st));
  {
    // products of a batch of 16 words: 45 and the power's squarings and set exponent bits; six FP64 instructions each (f64mod.hpp)
    double products = 0;
    for (int i = 0; i < ctx->L; i++) products += 45.0 + (ctx->use_int ? 62 : 52) + __builtin_popcountll(ctx->q[i] - 2);
    const double batches = (double)count * (double)ctx->N / 16.0;
    ProfScope prof(ctx, st, "ring_inv_or_zero_kernel", (d_num ? 3.0 : 2.0) * (double)count * (double)words * 8,
                   ctx->use_int ? 0.0 : 6.0 * products * batches);
    // non-temporal stores once the output is larger than the caches (the rule of launch_pointwise_arith, rs_core.hip)
    const bool nt = count * words * 8 >= ((size_t)64 << 20);
    dispatch_arith(ctx, [&](auto tag) {
      using M = decltype(tag);
      if (d_num) inv_launch<M, true>(ctx, x, num, out, a, nt, blocks, rep, st);
      else inv_launch<M, false>(ctx, x, num, out, a, nt, blocks, rep, st);
    });
  }
  RS_HIP(hipGetLastError());
  hipLaunchKernelGGL(ring_inv_or_zero_finish_kernel, dim3(1), dim3(64), 0, st, x, num, a, rep);
  RS_HIP(hipGetLastError());
  if (h_report) {
    unsigned long long h[INV_WORDS];
    RS_HIP(hipMemcpyAsync(h, rep, sizeof(h), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    r.n_zero = h[2];
    if (h[0] != ~0ull) {
      const size_t idx = (size_t)(h[0] % words);
      r.zero_elem = (uint64_t)(h[0] / words);
      r.zero_limb = (uint32_t)(idx / (size_t)ctx->N);
      r.zero_slot = (uint32_t)(idx % (size_t)ctx->N);
    }
    r.n_bad = h[3];
    if (h[1] != ~0ull) {
      const size_t idx = (size_t)(h[1] % words);
      r.bad_elem = (uint64_t)(h[1] / words);
      r.bad_limb = (uint32_t)(idx / (size_t)ctx->N);
      r.bad_slot = (uint32_t)(idx % (size_t)ctx->N);
      r.bad_x = h[4];
      r.bad_num = h[5];
    }
    *h_report = r;
  }
  RS_API_END
}

}  // extern "C"
