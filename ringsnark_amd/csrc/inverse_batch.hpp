// inverse_batch.hpp -- the device pieces of the batched inverse that inverse.hip and r1cs_hints.hip share: the working domain
// of a batch, the Fermat power, Montgomery's trick on a register array, and a workgroup's tallies into four report words
#pragma once
#include "rs_internal.hpp"

namespace rs {

// what a lane has seen over its pieces
struct InvTally {
  unsigned long long nz = 0, nb = 0, kz = ~0ull, kb = ~0ull;  // zeros, bad positions, the smallest key of each
};

// The working domain of a batch: centred doubles (FP64), Montgomery form (integers); mulmod of two values of the domain is
// a value of the domain in both (f64mod.hpp: |a b| <= 0.875^2 p^2 < p 2^50; intmod.hpp: REDC(aR bR) = abR).
template <class M>
__device__ __forceinline__ typename ArithOf<M>::T inv_enter(uint64_t w, const M &m) {
  using T = typename ArithOf<M>::T;
  return to_mont(center(from_res<T>(w), m), m);
}
// x^(p - 2): the loop of ring_inv_kernel / ring_inv_kernel_int; the exponent is uniform, so its bits branch on the scalar unit
template <class M>
__device__ __forceinline__ typename ArithOf<M>::T inv_fermat(typename ArithOf<M>::T base, typename ArithOf<M>::T one, const M &m) {
  const uint64_t e = modulus_u64(m) - 2;
  typename ArithOf<M>::T acc = one;
  constexpr int BITS = sizeof(M) == sizeof(Mod) ? 52 : 62;
  for (int bit = 0; bit < BITS; bit++) {
    if ((e >> bit) & 1ull) acc = mulmod(acc, base, m);
    base = mulmod(base, base, m);
  }
  return acc;
}

// The inverses of NW words of the domain, none of them zero, with ONE Fermat power (Montgomery's trick): 3 (NW - 1) products
// beside it.  f is replaced by the inverses, values of the domain.
template <class M, int NW>
__device__ __forceinline__ void inv_batch(typename ArithOf<M>::T (&f)[NW], const M &m) {
  using T = typename ArithOf<M>::T;
  T p[NW];
  p[0] = f[0];
#pragma unroll
  for (int u = 1; u < NW; u++) p[u] = mulmod(p[u - 1], f[u], m);
  T inv = inv_fermat<M>(p[NW - 1], inv_enter<M>(1ull, m), m);
#pragma unroll
  for (int u = NW - 1; u > 0; u--) {
    const T r = mulmod(inv, p[u - 1], m);
    inv = mulmod(inv, f[u], m);
    f[u] = r;
  }
  f[0] = inv;
}

// The tallies of a workgroup into the report words: waves by shuffles, the four waves through LDS, one lane issues the atomics.
__device__ __forceinline__ void inv_report(InvTally t, unsigned long long *__restrict__ rep) {
  __shared__ unsigned long long sh[4][4];
  if (!__syncthreads_or((t.nz | t.nb) != 0ull)) return;  // uniform over the workgroup: the common path ends here
  for (int d = 32; d >= 1; d >>= 1) {
    t.nz += __shfl_xor(t.nz, d);
    t.nb += __shfl_xor(t.nb, d);
    const unsigned long long oz = __shfl_xor(t.kz, d), ob = __shfl_xor(t.kb, d);
    t.kz = oz < t.kz ? oz : t.kz;
    t.kb = ob < t.kb ? ob : t.kb;
  }
  if ((threadIdx.x & 63u) == 0) {
    unsigned long long *w = sh[threadIdx.x >> 6];
    w[0] = t.nz, w[1] = t.nb, w[2] = t.kz, w[3] = t.kb;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < 4; k++) {
    t.nz += sh[k][0];
    t.nb += sh[k][1];
    t.kz = sh[k][2] < t.kz ? sh[k][2] : t.kz;
    t.kb = sh[k][3] < t.kb ? sh[k][3] : t.kb;
  }
  if (t.nz) {
    atomicAdd(rep + 2, t.nz);
    if (t.kz < __hip_atomic_load(rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rep, t.kz);
  }
  if (t.nb) {
    atomicAdd(rep + 3, t.nb);
    if (t.kb < __hip_atomic_load(rep + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rep + 1, t.kb);
  }
}

}  // namespace rs
