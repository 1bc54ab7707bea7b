// r1cs_hints.hip -- the assignment solver with hints (include/ringsnark_amd/solve_hints.h): bit, inverse-or-zero and quotient
// wires of wires the solver itself produces, as steps of one plan.
//
// The schedule is build_schedule of r1cs_solve.hip with the hint list; a hint step sits in the step arrays as a constraint
// step does (index = the hint, wire = its first target) with a kind byte beside it, and the hint steps of a level follow its
// constraint steps.  Constraint steps run on the kernels of r1cs_solve.hip, launched through solve_launch; two kernels are new:
//   solve_hint_level_kernel  the hint steps of ONE level, grid (slot chunks x groups of HINT_GROUP steps).  A thread owns one
//                            slot pair; the INV and QUOT steps of its group share one Fermat power (Montgomery's trick over
//                            2 * HINT_GROUP words); a BITS step reads the limb-0 words of its source, which ANOTHER workgroup
//                            of a lower level's launch stored: stream order is all the ordering it needs
//   solve_walk_hint_kernel   solve_walk_kernel with INV and QUOT hint steps inline: both are slot-local, so the thread still
//                            re-reads only words it stored itself; one Fermat power per step for the pair.  Never a BITS step:
//                            build_launches ends the walk run there, in every mode
// No kernel waits on another workgroup.  Every index into the assignment comes from the plan, the hint table and the CSR,
// all validated on the host; none is computed from assignment data.
//
// The report (four words the plan owns: key of the first zero source, key of the first bad bit position, zeros, bad positions)
// is that of inverse.hip: tallies in registers, reduced once per workgroup, no atomic on clean input; key = hint << 32 |
// limb * N + slot, so one 64-bit atomicMin orders by hint and then by position.
#include <algorithm>
#include <string>

#include "../../include/ringsnark_amd/solve_hints.h"
#include "inverse_batch.hpp"
#include "r1cs_solve_dev.hpp"
#include "r1cs_solve_plan.hpp"

struct rs_r1cs_hint_plan {
  rs_r1cs_solve_plan base;  // context, system, the steps and their device arrays; base.info and base.launches are not used
  rs_r1cs_hint_info info{};
  std::vector<rs_solve_hint> hints;
  std::vector<uint8_t> kinds;  // [n_steps]
  std::vector<rs::SolveLaunch> launches[3];  // by mode; kind 3: a walk run that holds hint steps (solve_walk_hint_kernel)
  rs_solve_hint *d_hints = nullptr;
  uint8_t *d_kinds = nullptr;
  unsigned long long *d_report = nullptr;
};

namespace rs {

constexpr size_t HINT_FILL_WORKGROUPS = 256;  // SOLVE_FILL_WORKGROUPS of r1cs_solve.hip: the AUTO rule is the same rule
constexpr int HINT_GROUP = 4;                 // hint steps of a level per workgroup: up to 8 words behind one Fermat power
constexpr int HINT_REPORT_WORDS = 4;

// BITS for one slot pair of limb `limb`: the bits of the limb-0 words into every target row, this limb's words compared
template <class M>
__device__ __forceinline__ void hint_bits_pair(const rs_solve_hint &h, uint32_t hint, uint64_t *asg, size_t S, size_t pair, int limb, int N,
                                               InvTally &tally) {
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(asg + (size_t)h.src * S);
  const ulonglong2 v = src[pair - (size_t)limb * (size_t)(N / 2)], w = src[pair];
  for (uint32_t k = 0; k < h.nbits; k++) {
    ulonglong2 o;
    o.x = (v.x >> k) & 1ull;
    o.y = (v.y >> k) & 1ull;
    reinterpret_cast<ulonglong2 *>(asg + ((size_t)h.dst + (size_t)k * h.dst_stride) * S)[pair] = o;
  }
  const bool b0 = limb ? w.x != v.x : (v.x >> h.nbits) != 0, b1 = limb ? w.y != v.y : (v.y >> h.nbits) != 0;
  if (b0 || b1) {
    tally.nb += (b0 ? 1 : 0) + (b1 ? 1 : 0);
    const unsigned long long key = (unsigned long long)hint << 32 | (2 * pair + (b0 ? 0 : 1));
    tally.kb = key < tally.kb ? key : tally.kb;
  }
}

// the source words of an INV or QUOT step for one slot pair: zeros noted in the tally and replaced by 1
__device__ __forceinline__ ulonglong2 hint_inv_load(const rs_solve_hint &h, uint32_t hint, const uint64_t *asg, size_t S, size_t pair, bool &z0,
                                                    bool &z1, InvTally &tally) {
  ulonglong2 x = reinterpret_cast<const ulonglong2 *>(asg + (size_t)h.src * S)[pair];
  z0 = x.x == 0ull;
  z1 = x.y == 0ull;
  if (z0 || z1) {
    tally.nz += (z0 ? 1 : 0) + (z1 ? 1 : 0);
    const unsigned long long key = (unsigned long long)hint << 32 | (2 * pair + (z0 ? 0 : 1));
    tally.kz = key < tally.kz ? key : tally.kz;
    if (z0) x.x = 1ull;
    if (z1) x.y = 1ull;
  }
  return x;
}

// out of the domain and into the target row: times the numerator as a data word (QUOT), or times 1 (INV)
template <class M>
__device__ __forceinline__ void hint_inv_store(const rs_solve_hint &h, typename ArithOf<M>::T r0, typename ArithOf<M>::T r1, bool z0, bool z1,
                                               uint64_t *asg, size_t S, size_t pair, const M &mod) {
  using T = typename ArithOf<M>::T;
  ulonglong2 o;
  if (h.kind == RS_HINT_QUOT) {
    const ulonglong2 n = reinterpret_cast<const ulonglong2 *>(asg + (size_t)h.num * S)[pair];
    o.x = to_res(canon(mulmod(center(from_res<T>(n.x), mod), r0, mod), mod));
    o.y = to_res(canon(mulmod(center(from_res<T>(n.y), mod), r1, mod), mod));
  } else {
    o.x = to_res(canon(konst_value(r0, mod), mod));
    o.y = to_res(canon(konst_value(r1, mod), mod));
  }
  if (z0) o.x = 0ull;
  if (z1) o.y = 0ull;
  reinterpret_cast<ulonglong2 *>(asg + (size_t)h.dst * S)[pair] = o;
}

// grid: (slot chunks of 256 slot pairs) x (groups of HINT_GROUP hint steps of the level [s_lo, s_hi)), one dimension, ordered
// by xcd_position.  The rows read (levels below) and the rows written (this level) are disjoint.  rep == nullptr: no report.
template <class M>
__global__ void __launch_bounds__(256)
solve_hint_level_kernel(const uint32_t *__restrict__ step_index, const rs_solve_hint *__restrict__ hints, size_t s_lo, size_t s_hi, uint64_t *asg,
                        int N, int L, const M *__restrict__ qmod, unsigned n_groups, unsigned long long *__restrict__ rep) {
  using T = typename ArithOf<M>::T;
  const unsigned pos = xcd_position(blockIdx.x, gridDim.x);
  const unsigned chunk = pos / n_groups, group = pos % n_groups;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)chunk * 256 + threadIdx.x;
  const bool live = 2 * pair < S;  // no early return: the report is a workgroup's
  const int limb = live ? (int)((2 * pair) / (size_t)N) : 0;
  const M mod = qmod[limb];
  const size_t lo = s_lo + (size_t)group * HINT_GROUP;
  InvTally tally;
  // the steps of the group are wave-uniform; words of the batch that no INV / QUOT step fills are factors 1
  rs_solve_hint h[HINT_GROUP];
  bool inv[HINT_GROUP], z0[HINT_GROUP], z1[HINT_GROUP];
  T f[2 * HINT_GROUP];
  const T one = inv_enter<M>(1ull, mod);
  bool any = false;
#pragma unroll
  for (int u = 0; u < HINT_GROUP; u++) {
    inv[u] = z0[u] = z1[u] = false;
    f[2 * u] = f[2 * u + 1] = one;
    if (lo + u >= s_hi) continue;
    const uint32_t hint = step_index[lo + u];
    h[u] = hints[hint];
    if (h[u].kind == RS_HINT_BITS) {
      if (live) hint_bits_pair<M>(h[u], hint, asg, S, pair, limb, N, tally);
      continue;
    }
    inv[u] = any = true;
    if (live) {
      const ulonglong2 x = hint_inv_load(h[u], hint, asg, S, pair, z0[u], z1[u], tally);
      f[2 * u] = inv_enter<M>(x.x, mod);
      f[2 * u + 1] = inv_enter<M>(x.y, mod);
    }
  }
  if (any) {
    inv_batch<M, 2 * HINT_GROUP>(f, mod);
#pragma unroll
    for (int u = 0; u < HINT_GROUP; u++)
      if (inv[u] && live) hint_inv_store<M>(h[u], f[2 * u], f[2 * u + 1], z0[u], z1[u], asg, S, pair, mod);
  }
  if (rep) inv_report(tally, rep);
}

// grid: slot chunks.  solve_walk_kernel (r1cs_solve.hip) with INV and QUOT hint steps inline: what a step reads was given or
// was stored by this very thread in an earlier step, hint steps included, so program order is all the ordering there is.
template <class M>
__global__ void __launch_bounds__(256)
solve_walk_hint_kernel(const SolveCsr<typename ArithOf<M>::T> cs, const uint32_t *__restrict__ step_index, const uint32_t *__restrict__ step_wire,
                       const uint8_t *__restrict__ step_kind, const typename ArithOf<M>::T *__restrict__ kinv /* [L][n_steps] */, size_t n_steps,
                       const rs_solve_hint *__restrict__ hints, size_t s_lo, size_t s_hi, uint64_t *asg, int N, int L,
                       const M *__restrict__ qmod, unsigned long long *__restrict__ rep) {
  using T = typename ArithOf<M>::T;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = 2 * pair < S;  // no early return: the report is a workgroup's
  const int limb = live ? (int)((2 * pair) / (size_t)N) : 0;
  const M mod = qmod[limb];
  const T *kinv_limb = kinv + (size_t)limb * n_steps;
  InvTally tally;
  for (size_t s = s_lo; s < s_hi; s++) {
    if (step_kind[s] == 0) {  // wave-uniform
      if (live) solve_step<M>(cs, load_step(cs, step_index, step_wire, kinv_limb, s), asg, S, pair, limb, mod);
      continue;
    }
    const uint32_t hint = step_index[s];
    const rs_solve_hint h = hints[hint];
    if (h.kind == RS_HINT_BITS || !live) continue;  // a BITS step is never in a walk run (build_launches)
    bool z0, z1;
    const ulonglong2 x = hint_inv_load(h, hint, asg, S, pair, z0, z1, tally);
    T f[2] = {inv_enter<M>(x.x, mod), inv_enter<M>(x.y, mod)};
    inv_batch<M, 2>(f, mod);
    hint_inv_store<M>(h, f[0], f[1], z0, z1, asg, S, pair, mod);
  }
  if (rep) inv_report(tally, rep);
}

static size_t hint_targets(const rs_solve_hint &h) { return h.kind == RS_HINT_BITS ? (size_t)h.nbits : (size_t)1; }
static size_t hint_stride(const rs_solve_hint &h) { return h.kind == RS_HINT_BITS ? (size_t)h.dst_stride : (size_t)1; }

// every refusal of solve_hints.h, before anything is allocated on the device
static void validate_hints(const rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given, const rs_solve_hint *hints, size_t n_hints) {
  const size_t nv = cs->n_vars;
  RS_REQUIRE(n_hints < 0xFFFFFFFFull, "too many hints");
  int max_bits = 63;
  for (int i = 0; i < ctx->L; i++) {
    int lg = 0;
    while (lg < 63 && (ctx->q[i] >> (lg + 1)) != 0) lg++;
    max_bits = std::min(max_bits, lg);
  }
  std::vector<uint8_t> taken(nv, 0);
  for (size_t i = 0; i < n_hints; i++) {
    const rs_solve_hint &h = hints[i];
    const std::string at = "hint " + std::to_string(i) + ": ";
    RS_REQUIRE(h.kind == RS_HINT_BITS || h.kind == RS_HINT_INV || h.kind == RS_HINT_QUOT, at + "unknown kind");
    RS_REQUIRE(h.src < nv && h.dst < nv && (h.kind != RS_HINT_QUOT || h.num < nv), at + "variable out of range");
    if (h.kind == RS_HINT_BITS) {
      RS_REQUIRE(h.nbits >= 1 && h.nbits <= (uint32_t)max_bits, at + "nbits must be between 1 and min_i floor(log2 q_i) = " + std::to_string(max_bits));
      RS_REQUIRE(h.dst_stride >= 1, at + "dst_stride must be at least 1");
      RS_REQUIRE((size_t)h.dst + (size_t)(h.nbits - 1) * h.dst_stride < nv, at + "variable out of range");
    }
    for (size_t t = 0; t < hint_targets(h); t++) {
      const size_t v = (size_t)h.dst + t * hint_stride(h);
      RS_REQUIRE(!h_given[v], at + "target " + std::to_string(v) + " is given");
      RS_REQUIRE(!taken[v], at + "target " + std::to_string(v) + " is named twice");
      RS_REQUIRE(v != h.src && (h.kind != RS_HINT_QUOT || v != h.num), at + "a source is among its own targets");
      taken[v] = 1;
    }
  }
}

// The launches of every mode (solve_hints.h).  Per level: the constraint steps [clo, hlo), the hint steps [hlo, hi).
static void build_hint_launches(const rs_ctx *ctx, rs_r1cs_hint_plan *P) {
  const std::vector<uint64_t> &lp = P->base.level_ptr;
  const size_t n_levels = lp.size() - 1, n_steps = P->kinds.size();
  const size_t chunks = (ctx->ring_words() / 2 + 255) / 256;
  for (auto &l : P->launches) l.clear();
  if (n_steps == 0 || chunks == 0) return;
  auto as_levels = [&](std::vector<SolveLaunch> &list, size_t clo, size_t hlo, size_t hi) {
    if (hlo > clo) list.push_back(SolveLaunch{0, clo, hlo, 0, 0});
    if (hi > hlo) list.push_back(SolveLaunch{2, hlo, hi, 0, 0});
  };
  auto walk_to = [&](std::vector<SolveLaunch> &list, size_t lo, size_t hi) {  // extends the walk run that ends at lo, or starts one
    if (hi == lo) return;
    if (!list.empty() && (list.back().kind == 1 || list.back().kind == 3) && list.back().s_hi == lo) list.back().s_hi = hi;
    else list.push_back(SolveLaunch{1, lo, hi, 0, 0});
  };
  auto as_walk = [&](std::vector<SolveLaunch> &list, size_t clo, size_t hlo, size_t hi) {
    bool bits = false;
    for (size_t s = hlo; s < hi; s++) bits |= P->hints[P->base.rows[s]].kind == RS_HINT_BITS;
    if (!bits) return walk_to(list, clo, hi);
    walk_to(list, clo, hlo);  // a BITS step ends the run; the level's hint steps go to the hint-level kernel together
    list.push_back(SolveLaunch{2, hlo, hi, 0, 0});
  };
  for (size_t l = 0; l < n_levels; l++) {
    const size_t clo = lp[l], hi = lp[l + 1];
    size_t hlo = clo;
    while (hlo < hi && P->kinds[hlo] == 0) hlo++;
    for (size_t s = hlo; s < hi; s++) RS_REQUIRE(P->kinds[s] == 1, "hint steps do not follow the constraint steps of their level");
    as_levels(P->launches[RS_SOLVE_LEVELS], clo, hlo, hi);
    as_walk(P->launches[RS_SOLVE_WALK], clo, hlo, hi);
    if ((hi - clo) * chunks >= HINT_FILL_WORKGROUPS) as_levels(P->launches[RS_SOLVE_AUTO], clo, hlo, hi);
    else as_walk(P->launches[RS_SOLVE_AUTO], clo, hlo, hi);
  }
  // costs: constraint steps as r1cs_solve.hip counts them; a hint step reads its sources and writes its targets, and an
  // inverse is about 10 products and the power's squarings for a slot pair
  std::vector<uint32_t> seen(P->base.cs->n_vars + 1, 0);
  uint32_t token = 0;
  const double Sw = (double)ctx->ring_words();
  for (auto &list : P->launches)
    for (SolveLaunch &ln : list) {
      double bytes = 0, ops = 0;
      for (size_t s = ln.s_lo; s < ln.s_hi;) {
        if (P->kinds[s]) {
          const rs_solve_hint &h = P->hints[P->base.rows[s]];
          if (h.kind != RS_HINT_BITS) ln.kind = ln.kind == 1 ? 3 : ln.kind;
          bytes += (double)((h.kind == RS_HINT_QUOT ? 2 : 1) + hint_targets(h)) * Sw * 8 + sizeof(rs_solve_hint) + 5;
          ops += h.kind == RS_HINT_BITS ? 0.0 : 7.0 * (10 + (ctx->use_int ? 62 : 52) * 1.5) * Sw / 2;
          s++;
          continue;
        }
        SolveLaunch part{0, s, s, 0, 0};
        while (part.s_hi < ln.s_hi && P->kinds[part.s_hi] == 0) part.s_hi++;
        launch_cost(ctx, &P->base, seen, ++token, part);
        bytes += part.bytes;
        ops += part.ops;
        s = part.s_hi;
      }
      ln.bytes = bytes;
      ln.ops = ops;
      if (ln.kind == 1 || ln.kind == 3)
        for (size_t s = ln.s_lo; s < ln.s_hi; s++)
          RS_REQUIRE(!P->kinds[s] || P->hints[P->base.rows[s]].kind != RS_HINT_BITS, "a BITS hint step inside a walk run");
    }
}

template <class M>
static void hint_launch_arith(rs_ctx *ctx, const rs_r1cs_hint_plan *P, uint64_t *d_asg, const SolveLaunch &ln, unsigned long long *rep,
                              hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const size_t chunks = (ctx->ring_words() / 2 + 255) / 256;
  if (ln.kind == 2) {
    const size_t groups = (ln.s_hi - ln.s_lo + HINT_GROUP - 1) / HINT_GROUP;
    RS_REQUIRE(chunks * groups < ((size_t)1 << 31), "level too wide for one launch of the solver");
    ProfScope p(ctx, st, "solve_hint_level", ln.bytes, ln.ops);
    hipLaunchKernelGGL(solve_hint_level_kernel<M>, dim3((unsigned)(chunks * groups)), dim3(256), 0, st, P->base.d_rows, P->d_hints, ln.s_lo, ln.s_hi,
                       d_asg, ctx->N, ctx->L, CtxArith<M>::qmod(ctx), (unsigned)groups, rep);
  } else {
    const rs_r1cs *cs = P->base.cs;
    SolveCsr<T> k;
    for (int w = 0; w < 3; w++) {
      k.rp[w] = cs->d_row_ptr[w];
      k.col[w] = cs->d_col[w];
      k.cf[w] = reinterpret_cast<const T *>(cs->d_coeff[w]);
      k.nnz[w] = cs->nnz[w];
      k.px[w] = cs->d_pidx[w];
    }
    k.ptab = reinterpret_cast<const T *>(cs->d_ptab);
    ProfScope p(ctx, st, "solve_walk_hint", ln.bytes, ln.ops);
    hipLaunchKernelGGL(solve_walk_hint_kernel<M>, dim3((unsigned)chunks), dim3(256), 0, st, k, P->base.d_rows, P->base.d_wires, P->d_kinds,
                       reinterpret_cast<const T *>(P->base.d_kinv), P->kinds.size(), P->d_hints, ln.s_lo, ln.s_hi, d_asg, ctx->N, ctx->L,
                       CtxArith<M>::qmod(ctx), rep);
  }
  RS_HIP(hipGetLastError());
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_r1cs_hint_plan_create(rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given, const rs_solve_hint *h_hints, size_t n_hints,
                             rs_r1cs_hint_plan **out, rs_r1cs_hint_info *h_info) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(cs && out && (h_given || cs->n_vars == 0) && (h_hints || n_hints == 0), "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  RS_REQUIRE(ctx->N >= 2 && ctx->N % 2 == 0 && ctx->ring_words() < ((size_t)1 << 32), "ring too large for the positions of the hint report");
  validate_hints(ctx, cs, h_given, h_hints, n_hints);
  struct Holder {  // frees a partly built plan when a check below throws
    rs_r1cs_hint_plan *p;
    ~Holder() { rs_r1cs_hint_plan_destroy(p); }
  } holder{new rs_r1cs_hint_plan()};
  rs_r1cs_hint_plan *P = holder.p;
  P->base.ctx = ctx;
  P->base.cs = cs;
  P->hints.assign(h_hints, h_hints + n_hints);
  std::vector<uint64_t> k;
  HintSchedule hs;
  build_schedule(ctx, cs, h_given, &P->base, k, n_hints ? P->hints.data() : nullptr, n_hints, &hs);
  P->kinds = hs.kinds;
  P->kinds.resize(P->base.rows.size(), 0);  // no hints: the scheduler left hs alone
  P->info.solve = P->base.info;
  P->info.n_steps = P->base.rows.size();
  P->info.n_hints_run = hs.n_run;
  P->info.n_hints_blocked = hs.n_blocked;
  P->info.first_blocked_hint = n_hints ? hs.first_blocked : 0;
  upload_schedule(ctx, &P->base, k, P->kinds.data(), n_hints);
  if (!P->kinds.empty()) {
    RS_HIP(hipMalloc(&P->d_kinds, P->kinds.size()));
    RS_HIP(hipMemcpy(P->d_kinds, P->kinds.data(), P->kinds.size(), hipMemcpyHostToDevice));
  }
  if (n_hints) {
    RS_HIP(hipMalloc(&P->d_hints, sizeof(rs_solve_hint) * n_hints));
    RS_HIP(hipMemcpy(P->d_hints, P->hints.data(), sizeof(rs_solve_hint) * n_hints, hipMemcpyHostToDevice));
    RS_HIP(hipMalloc(&P->d_report, sizeof(unsigned long long) * HINT_REPORT_WORDS));
  }
  build_hint_launches(ctx, P);
  if (h_info) *h_info = P->info;
  holder.p = nullptr;
  *out = P;
  RS_API_END
}

int rs_r1cs_hint_plan_steps(const rs_r1cs_hint_plan *plan, uint8_t *h_kind, uint32_t *h_index, uint32_t *h_wire, uint64_t *h_level_ptr) {
  RS_API_BEGIN
  RS_REQUIRE(plan, "null argument");
  if (h_kind) std::copy(plan->kinds.begin(), plan->kinds.end(), h_kind);
  if (h_index) std::copy(plan->base.rows.begin(), plan->base.rows.end(), h_index);
  if (h_wire) std::copy(plan->base.wires.begin(), plan->base.wires.end(), h_wire);
  if (h_level_ptr) std::copy(plan->base.level_ptr.begin(), plan->base.level_ptr.end(), h_level_ptr);
  RS_API_END
}

void rs_r1cs_hint_plan_destroy(rs_r1cs_hint_plan *plan) {
  if (!plan) return;
  if (plan->base.d_rows) (void)hipFree(plan->base.d_rows);
  if (plan->base.d_wires) (void)hipFree(plan->base.d_wires);
  if (plan->base.d_kinv) (void)hipFree(plan->base.d_kinv);
  if (plan->d_kinds) (void)hipFree(plan->d_kinds);
  if (plan->d_hints) (void)hipFree(plan->d_hints);
  if (plan->d_report) (void)hipFree(plan->d_report);
  delete plan;
}

int rs_r1cs_solve_hinted(rs_ctx *ctx, const rs_r1cs_hint_plan *plan, uint64_t *d_assignment, int mode, rs_r1cs_hint_stats *h_stats,
                         rs_solve_hint_report *h_report, rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(plan && d_assignment, "null argument");
  RS_REQUIRE(plan->base.ctx == ctx, "solve plan of another context");
  RS_REQUIRE(mode == RS_SOLVE_AUTO || mode == RS_SOLVE_LEVELS || mode == RS_SOLVE_WALK, "unknown solve mode");
  const std::vector<SolveLaunch> &launches = plan->launches[mode];
  rs_r1cs_hint_stats stats{0, 0, 0};
  bool any_hint = false;
  for (const SolveLaunch &ln : launches) {
    (ln.kind == 0 ? stats.level_launches : ln.kind == 2 ? stats.hint_launches : stats.walk_launches)++;
    any_hint |= ln.kind >= 2;
  }
  hipStream_t st = S(stream);
  unsigned long long *rep = h_report && any_hint ? plan->d_report : nullptr;
  if (rep) {
    RS_HIP(hipMemsetAsync(rep, 0, sizeof(unsigned long long) * HINT_REPORT_WORDS, st));
    RS_HIP(hipMemsetAsync(rep, 0xFF, sizeof(unsigned long long) * 2, st));
  }
  if (!launches.empty()) {
    std::unique_lock<std::mutex> lk(ctx->mu, std::defer_lock);
    if (ctx->profiling) lk.lock();  // the record ProfScope appends to belongs to the holder of mu
    for (const SolveLaunch &ln : launches) {
      if (ln.kind < 2) solve_launch(ctx, &plan->base, d_assignment, ln, st);
      else dispatch_arith(ctx, [&](auto tag) { hint_launch_arith<decltype(tag)>(ctx, plan, d_assignment, ln, rep, st); });
    }
  }
  if (h_report) {
    rs_solve_hint_report r{};
    unsigned long long h[HINT_REPORT_WORDS] = {~0ull, ~0ull, 0, 0};
    if (rep) RS_HIP(hipMemcpyAsync(h, rep, sizeof(h), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    const uint64_t N = (uint64_t)ctx->N;
    r.n_zero = h[2];
    if (h[0] != ~0ull) {
      r.zero_hint = (uint32_t)(h[0] >> 32);
      r.zero_limb = (uint32_t)((h[0] & 0xFFFFFFFFull) / N);
      r.zero_slot = (uint32_t)((h[0] & 0xFFFFFFFFull) % N);
    }
    r.n_bits_bad = h[3];
    if (h[1] != ~0ull) {
      r.bad_hint = (uint32_t)(h[1] >> 32);
      r.bad_limb = (uint32_t)((h[1] & 0xFFFFFFFFull) / N);
      r.bad_slot = (uint32_t)((h[1] & 0xFFFFFFFFull) % N);
    }
    *h_report = r;
  }
  if (h_stats) *h_stats = stats;
  RS_API_END
}

}  // extern "C"
