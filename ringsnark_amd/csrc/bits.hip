// bits.hip -- rs_ring_bit_decompose (include/ringsnark_amd/bits.h): the bit rows of ring elements whose slots hold one
// integer v < 2^nbits in every limb -- the wires of a range check that no constraint determines forwards.
//
// A write-dominated stream: per slot one word is read from limb 0 (and one per further limb, to compare) and nbits * L words
// are written.  Integers only, so the two arithmetics of a context share this one kernel.
//
// Every reported field is a function of the inputs only:
//   n_bad        integer atomicAdd of per-wave counts of bad positions
//   first        64-bit atomicMin over the key element * L*N + limb * N + slot (the minimum does not depend on arrival order)
//   word, value  two loads at the minimal key, by the second kernel
// The common path -- clean input -- issues no atomic: a wave votes on one flag per piece and goes on.
#include <cstdint>
#include <string>

#include "../../include/ringsnark_amd/bits.h"
#include "rs_internal.hpp"

namespace rs {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));  // as in ntt_wide.hpp

// The access shape of ring_pointwise_kernel (rs_core.hip): a workgroup takes a PIECE of 256 * 8 consecutive slot pairs (16-byte
// words of limb 0; consecutive elements follow each other in this numbering), eight 16-byte loads per lane in flight before
// the first use, pieces dealt round-robin to the workgroups.  For every (bit, limb) a piece then writes the same slot pairs of
// one output row: 32 KiB contiguous wherever a limb row holds a piece (N >= 4096), whole limb rows otherwise.
constexpr int BITS_U = 8;
constexpr size_t BITS_PIECE = (size_t)256 * BITS_U;
// device side of the report: [0] key of the first bad position (all ones: none), [1] bad positions, [2] word, [3] value there
constexpr int BITS_WORDS = 4;

// x: limb 0 of element 0; bits: bit row 0 of element 0 -- kernel parameters of their own, so that they are global pointers
struct BitsArgs {
  size_t total;      // count * P slot pairs
  size_t xs, bs;     // x_stride, bits_stride in 16-byte words: stride * L * P
  int logP, L, nbits;  // P = N / 2 slot pairs per limb row
};

// The rare path, entered by a whole wave when one of its lanes saw a bad word in the piece at `base`: reads the piece's input
// again (no output row shares a word with it), counts the bad positions and takes the smallest key.
__device__ __forceinline__ void bits_report_piece(const u64x2 *__restrict__ x, const BitsArgs &a, size_t base, unsigned long long *__restrict__ rep) {
  const size_t P = (size_t)1 << a.logP, S = 2 * P * (size_t)a.L;
  unsigned long long cnt = 0, key = ~0ull;
  for (int u = 0; u < BITS_U; u++) {
    const size_t t = base + threadIdx.x + 256 * u;
    if (t >= a.total) continue;
    const size_t e = t >> a.logP, p = t & (P - 1);
    const u64x2 *row = x + e * a.xs + p;
    const u64x2 v = row[0];
    for (int i = 0; i < a.L; i++) {
      const u64x2 w = row[(size_t)i * P];
      const bool bad1 = i ? w.y != v.y : (v.y >> a.nbits) != 0, bad0 = i ? w.x != v.x : (v.x >> a.nbits) != 0;
      const unsigned long long k = e * S + (size_t)i * 2 * P + 2 * p;
      if (bad1) cnt++, key = k + 1 < key ? k + 1 : key;
      if (bad0) cnt++, key = k < key ? k : key;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    cnt += __shfl_xor(cnt, d);
    const unsigned long long other = __shfl_xor(key, d);
    key = other < key ? other : key;
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicAdd(rep + 1, cnt);
    atomicMin(rep, key);
  }
}

// One piece.  GUARD: the last piece, which may end before its 2048th slot pair.
template <bool NT, bool GUARD>
__device__ __forceinline__ void bits_piece(const u64x2 *__restrict__ x, u64x2 *__restrict__ bits, const BitsArgs &a, size_t base,
                                           unsigned long long *__restrict__ rep) {
  const size_t P = (size_t)1 << a.logP;
  u64x2 v[BITS_U];
  size_t xo[BITS_U], bo[BITS_U];
  bool live[BITS_U];
#pragma unroll
  for (int u = 0; u < BITS_U; u++) {
    const size_t t = base + threadIdx.x + 256 * u;
    live[u] = !GUARD || t < a.total;
    const size_t e = t >> a.logP, p = t & (P - 1);
    xo[u] = e * a.xs + p;
    bo[u] = e * a.bs + p;
    v[u] = u64x2{0ull, 0ull};
    if (live[u]) v[u] = x[xo[u]];
  }
  unsigned long long anybad = 0;
#pragma unroll
  for (int u = 0; u < BITS_U; u++) anybad |= (v[u].x | v[u].y) >> a.nbits;
  for (int i = 1; i < a.L; i++) {  // the other limbs must repeat limb 0
    u64x2 w[BITS_U];
#pragma unroll
    for (int u = 0; u < BITS_U; u++) {
      w[u] = v[u];
      if (live[u]) w[u] = x[xo[u] + (size_t)i * P];
    }
#pragma unroll
    for (int u = 0; u < BITS_U; u++) anybad |= (w[u].x ^ v[u].x) | (w[u].y ^ v[u].y);
  }
  for (int k = 0; k < a.nbits; k++) {
    u64x2 o[BITS_U];
#pragma unroll
    for (int u = 0; u < BITS_U; u++) o[u] = u64x2{(v[u].x >> k) & 1ull, (v[u].y >> k) & 1ull};
    for (int i = 0; i < a.L; i++) {
      u64x2 *dst = bits + ((size_t)k * a.L + i) * P;
#pragma unroll
      for (int u = 0; u < BITS_U; u++) {
        if (!live[u]) continue;
        if (NT) __builtin_nontemporal_store(o[u], dst + bo[u]);
        else dst[bo[u]] = o[u];
      }
    }
  }
  if (__ballot(anybad != 0ull) == 0ull) return;  // wave-uniform: the common path ends here
  bits_report_piece(x, a, base, rep);
}

// NT: non-temporal stores (outputs larger than the caches they would otherwise sweep, written once)
template <bool NT>
__global__ void __launch_bounds__(256) ring_bit_decompose_kernel(const u64x2 *__restrict__ x, u64x2 *__restrict__ bits, BitsArgs a, size_t pieces,
                                                                 unsigned long long *__restrict__ rep) {
  for (size_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
    const size_t base = piece * BITS_PIECE;
    if (base + BITS_PIECE <= a.total) bits_piece<NT, false>(x, bits, a, base, rep);
    else bits_piece<NT, true>(x, bits, a, base, rep);
  }
}

// the two words at the first bad position
__global__ void ring_bit_decompose_finish_kernel(const u64x2 *__restrict__ x, BitsArgs a, unsigned long long *__restrict__ rep) {
  const unsigned long long key = rep[0];  // final: written by the launch before this one
  if (threadIdx.x != 0 || key == ~0ull) return;
  const size_t P = (size_t)1 << a.logP, S = 2 * P * (size_t)a.L;
  const size_t e = (size_t)(key / S), idx = (size_t)(key % S);
  const unsigned long long *row = reinterpret_cast<const unsigned long long *>(x + e * a.xs);
  rep[2] = row[idx];
  rep[3] = row[idx % (2 * P)];
}

// a * b, or RS_ERR_INVALID when the product does not fit
static size_t mul_fit(size_t a, size_t b) {
  size_t r = 0;
  RS_REQUIRE(!__builtin_mul_overflow(a, b, &r) && r < ((size_t)1 << 60), "count, strides and ring size address more than 2^60 words");
  return r;
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_ring_bit_decompose(rs_ctx *ctx, const uint64_t *d_x, size_t x_stride, size_t count, int nbits, uint64_t *d_bits,
                          size_t bits_stride, rs_bits_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  rs_bits_report out{};
  if (count == 0) {
    if (h_report) *h_report = out;
    return RS_OK;
  }
  RS_REQUIRE(d_x && d_bits, "null argument");
  int max_bits = 63;
  for (int i = 0; i < ctx->L; i++) {
    int lg = 0;
    while (lg < 63 && (ctx->q[i] >> (lg + 1)) != 0) lg++;
    max_bits = std::min(max_bits, lg);
  }
  RS_REQUIRE(nbits >= 1 && nbits <= max_bits,
             "nbits must be between 1 and min_i floor(log2 q_i) = " + std::to_string(max_bits) + " (every nbits-bit value a canonical residue in every limb)");
  RS_REQUIRE(x_stride >= 1, "x_stride must be at least 1 ring element");
  RS_REQUIRE(bits_stride >= (size_t)nbits, "bits_stride must be at least nbits = " + std::to_string(nbits) + " ring elements");
  int logN = 0;
  while ((1 << logN) < ctx->N) logN++;
  RS_REQUIRE((1 << logN) == ctx->N && logN >= 1, "ring degree must be a power of two, at least 2");
  RS_REQUIRE((((uintptr_t)d_x | (uintptr_t)d_bits) & 15u) == 0, "d_x and d_bits must be 16-byte aligned");
  const size_t words = ctx->ring_words(), P = (size_t)ctx->N / 2;
  // extents in words, then: no input row may share a word with an output row.  Both are ascending runs of disjoint intervals
  // (x_stride >= 1, bits_stride >= nbits), so one merge over the two decides it exactly.
  const size_t xs_words = mul_fit(x_stride, words), bs_words = mul_fit(bits_stride, words), out_words = mul_fit((size_t)nbits, words);
  const size_t x_extent = mul_fit(count - 1, xs_words) + words, b_extent = mul_fit(count - 1, bs_words) + out_words;
  const uintptr_t x0 = (uintptr_t)d_x, b0 = (uintptr_t)d_bits;
  RS_REQUIRE(x0 + 8 * x_extent > x0 && b0 + 8 * b_extent > b0, "count, strides and ring size address more than 2^60 words");
  if (!(x0 + 8 * x_extent <= b0 || b0 + 8 * b_extent <= x0)) {
    for (size_t i = 0, j = 0; i < count && j < count;) {
      const uintptr_t xi = x0 + 8 * i * xs_words, bj = b0 + 8 * j * bs_words;
      if (xi + 8 * words <= bj) i++;
      else if (bj + 8 * out_words <= xi) j++;
      else
        throw Error(RS_ERR_INVALID, "input element " + std::to_string(i) + " shares a word with the bit rows of element " + std::to_string(j) +
                                        ": no input row may overlap an output row");
    }
  }
  BitsArgs a{};
  const u64x2 *x = reinterpret_cast<const u64x2 *>(d_x);
  u64x2 *bits = reinterpret_cast<u64x2 *>(d_bits);
  a.total = mul_fit(count, P);
  a.xs = xs_words / 2;
  a.bs = bs_words / 2;
  a.logP = logN - 1;
  a.L = ctx->L;
  a.nbits = nbits;
  const size_t pieces = (a.total + BITS_PIECE - 1) / BITS_PIECE;
  const unsigned blocks = (unsigned)std::min<size_t>(pieces, 256 * 8);  // a bounded grid: the workgroups stride over the pieces
  hipStream_t st = S(stream);
  WsScope ws_scope(ctx, st);
  unsigned long long *rep = (unsigned long long *)ws_get(ctx, WS_SMALL, 256);
  RS_HIP(hipMemsetAsync(rep, 0, sizeof(unsigned long long) * BITS_WORDS, st));
  RS_HIP(hipMemsetAsync(rep, 0xFF, sizeof(unsigned long long), st));
  {
    ProfScope prof(ctx, st, "ring_bit_decompose_kernel", (1.0 + nbits) * (double)count * (double)words * 8, 0);
    // non-temporal stores once the output is larger than the caches (the rule of launch_pointwise_arith, rs_core.hip)
    if ((size_t)nbits * count * words * 8 >= ((size_t)64 << 20))
      hipLaunchKernelGGL(ring_bit_decompose_kernel<true>, dim3(blocks), dim3(256), 0, st, x, bits, a, pieces, rep);
    else
      hipLaunchKernelGGL(ring_bit_decompose_kernel<false>, dim3(blocks), dim3(256), 0, st, x, bits, a, pieces, rep);
  }
  RS_HIP(hipGetLastError());
  hipLaunchKernelGGL(ring_bit_decompose_finish_kernel, dim3(1), dim3(64), 0, st, x, a, rep);
  RS_HIP(hipGetLastError());
  if (h_report) {
    unsigned long long h[BITS_WORDS];
    RS_HIP(hipMemcpyAsync(h, rep, sizeof(h), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    out.n_bad = h[1];
    if (h[0] != ~0ull) {
      const size_t idx = (size_t)(h[0] % words);
      out.first_elem = (uint64_t)(h[0] / words);
      out.first_limb = (uint32_t)(idx / (size_t)ctx->N);
      out.first_slot = (uint32_t)(idx % (size_t)ctx->N);
      out.word = h[2];
      out.value = h[3];
    }
    *h_report = out;
  }
  RS_API_END
}

}  // extern "C"
