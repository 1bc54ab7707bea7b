// r1cs_solve.hip -- the assignment solver (include/ringsnark_amd/r1cs_solve.h): the full assignment [n_vars][L][N] of a
// forward-determined R1CS from its given wires, the step before rs_r1cs_check and the provers.
//
// A ring element in evaluation form is L*N independent residues, so solving the system is L*N independent scalar problems
// with ONE schedule.  The schedule is built on the host (build_schedule: unknown-counters per constraint and a wire ->
// constraint adjacency, O(nnz) apart from sorting each level's candidates); two kernels run it:
//   solve_level_kernel  one level per launch, grid (slot chunks x groups of steps): the steps of a level are independent, the
//                       levels are ordered by the stream
//   solve_walk_kernel   a run of consecutive levels per launch, grid slot chunks only: every thread walks the run's steps in
//                       order for its own slot pair and only ever re-reads words it stored itself (chain_kernel of
//                       prover.hip with the schedule read from memory)
// No kernel waits on another workgroup.  Every index into the assignment comes from the plan and the CSR, both validated
// on the host; none is computed from assignment data.
#include <algorithm>

#include "../../include/ringsnark_amd/r1cs_solve.h"
#include "r1cs_solve_dev.hpp"
#include "r1cs_solve_plan.hpp"

namespace rs {

// RS_SOLVE_AUTO: a level goes to the level kernel when its launch fills the device, width x slot chunks >= one workgroup
// per CU (256 CUs); consecutive narrower levels are merged into one walk launch.  A starting rule derived from the CU
// count, not a measured optimum (DESIGN.md "Assignment solver").
constexpr size_t SOLVE_FILL_WORKGROUPS = 256;
// steps per workgroup of the level kernel: as many as leave the device a few waves of workgroups (as CHECK's rows per workgroup)
constexpr size_t SOLVE_STEPS_PER_WG = 8;

// grid: (slot chunks of 256 slot pairs) x (groups of `spw` steps of the level [s_lo, s_hi)), one dimension, ordered by
// xcd_position.  A thread owns one slot pair.  The rows read (levels below) and the rows written (this level) are disjoint.
template <class M>
__global__ void __launch_bounds__(256)
solve_level_kernel(const SolveCsr<typename ArithOf<M>::T> cs, const uint32_t *__restrict__ step_row, const uint32_t *__restrict__ step_wire,
                   const typename ArithOf<M>::T *__restrict__ kinv /* [L][n_steps] */, size_t n_steps, size_t s_lo, size_t s_hi,
                   uint64_t *asg, int N, int L, const M *__restrict__ qmod, unsigned n_groups, unsigned spw) {
  const unsigned pos = xcd_position(blockIdx.x, gridDim.x);
  const unsigned chunk = pos / n_groups, group = pos % n_groups;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)chunk * 256 + threadIdx.x;
  if (2 * pair >= S) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const size_t lo = s_lo + (size_t)group * spw, hi = lo + spw < s_hi ? lo + spw : s_hi;
  for (size_t s = lo; s < hi; s++) solve_step<M>(cs, load_step(cs, step_row, step_wire, kinv + (size_t)limb * n_steps, s), asg, S, pair, limb, mod);
}

// grid: slot chunks.  Every thread walks the steps [s_lo, s_hi) in order for its own slot pair: what a step reads was given
// or was stored by this very thread in an earlier step, so program order is all the ordering there is -- `asg` is neither
// const nor restrict, and its loads are ordinary vector loads behind the thread's own stores.  The words of step s + 1 that
// do not depend on the assignment (schedule, row bounds, k^-1: wave-uniform) are loaded while step s computes; only the
// assignment loads sit on the dependent chain.
template <class M>
__global__ void __launch_bounds__(256)
solve_walk_kernel(const SolveCsr<typename ArithOf<M>::T> cs, const uint32_t *__restrict__ step_row, const uint32_t *__restrict__ step_wire,
                  const typename ArithOf<M>::T *__restrict__ kinv /* [L][n_steps] */, size_t n_steps, size_t s_lo, size_t s_hi,
                  uint64_t *asg, int N, int L, const M *__restrict__ qmod) {
  using T = typename ArithOf<M>::T;
  const size_t S = (size_t)L * N;
  const size_t pair = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (2 * pair >= S || s_lo >= s_hi) return;
  const int limb = (int)((2 * pair) / (size_t)N);
  const M mod = qmod[limb];
  const T *kinv_limb = kinv + (size_t)limb * n_steps;
  SolveStep<T> next = load_step(cs, step_row, step_wire, kinv_limb, s_lo);
  for (size_t s = s_lo; s < s_hi; s++) {
    const SolveStep<T> cur = next;
    if (s + 1 < s_hi) next = load_step(cs, step_row, step_wire, kinv_limb, s + 1);
    solve_step<M>(cs, cur, asg, S, pair, limb, mod);
  }
}

// The schedule of r1cs_solve.h, and with hints that of solve_hints.h (r1cs_solve_plan.hpp).  One body: a hint adds reserved
// wires, which no constraint step may take, and steps of its own, which become ready through a counter of unknown sources as
// a constraint does through its counters.
void build_schedule(const rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given, rs_r1cs_solve_plan *P, std::vector<uint64_t> &k,
                    const rs_solve_hint *hints, size_t n_hints, HintSchedule *hs) {
  const size_t m = cs->m, nv = cs->n_vars;
  const int L = ctx->L;
  RS_REQUIRE(m < ((size_t)1 << 31) && nv < 0xFFFFFFFFull, "constraint system too large for the solver");
  std::vector<uint8_t> known(nv);
  rs_r1cs_solve_info &info = P->info;
  info = rs_r1cs_solve_info{};
  for (size_t v = 0; v < nv; v++) info.n_given += (known[v] = h_given[v] ? 1 : 0);
  // distinct unknown wires per constraint, of a and b together and of c: counters, and the wire -> constraint adjacency
  // (entry 2 j + 1: the wire is in c of constraint j; 2 j: in a or b)
  std::vector<uint32_t> cnt_ab(m, 0), cnt_c(m, 0), c_ptr(m + 1, 0), c_list, adj_ptr(nv + 1, 0), adj;
  {
    std::vector<uint32_t> seen_ab(nv, ~0u), seen_c(nv, ~0u);
    std::vector<std::pair<uint32_t, uint32_t>> occ;  // (wire, adjacency entry)
    for (size_t j = 0; j < m; j++) {
      for (int w = 0; w < 3; w++)
        for (uint32_t e = cs->h_row_ptr[w][j]; e < cs->h_row_ptr[w][j + 1]; e++) {
          const uint32_t c = cs->h_col[w][e];
          if (c == 0 || known[c - 1]) continue;
          std::vector<uint32_t> &seen = w == 2 ? seen_c : seen_ab;
          if (seen[c - 1] == (uint32_t)j) continue;
          seen[c - 1] = (uint32_t)j;
          (w == 2 ? cnt_c : cnt_ab)[j]++;
          if (w == 2) c_list.push_back(c - 1);
          occ.emplace_back(c - 1, (uint32_t)(2 * j + (w == 2)));
          adj_ptr[c]++;
        }
      c_ptr[j + 1] = (uint32_t)c_list.size();
    }
    for (size_t v = 0; v < nv; v++) adj_ptr[v + 1] += adj_ptr[v];
    adj.resize(occ.size());
    std::vector<uint32_t> fill(adj_ptr.begin(), adj_ptr.end() - 1);
    for (const auto &o : occ) adj[fill[o.first]++] = o.second;
  }
  auto candidate = [&](size_t j) { return cnt_ab[j] == 0 && cnt_c[j] == 1; };
  std::vector<uint32_t> cand, next, fresh, claimed(nv, 0);
  // hints: the reserved wires, the unknown sources of every hint, and the wire -> hint adjacency of the sources
  auto targets = [&](size_t h) { return hints[h].kind == RS_HINT_BITS ? (size_t)hints[h].nbits : (size_t)1; };
  auto stride = [&](size_t h) { return hints[h].kind == RS_HINT_BITS ? (size_t)hints[h].dst_stride : (size_t)1; };
  std::vector<uint8_t> reserved, hint_done;
  std::vector<uint32_t> hcnt, hcand, hnext, hadj_ptr, hadj;
  if (n_hints) {
    reserved.assign(nv, 0);
    hint_done.assign(n_hints, 0);
    hcnt.assign(n_hints, 0);
    hadj_ptr.assign(nv + 1, 0);
    std::vector<std::pair<uint32_t, uint32_t>> occ;  // (wire, hint)
    for (size_t h = 0; h < n_hints; h++) {
      for (size_t t = 0; t < targets(h); t++) reserved[hints[h].dst + t * stride(h)] = 1;
      const uint32_t srcs[2] = {hints[h].src, hints[h].num};
      const int n_src = hints[h].kind == RS_HINT_QUOT && hints[h].num != hints[h].src ? 2 : 1;
      for (int i = 0; i < n_src; i++)
        if (!known[srcs[i]]) {
          hcnt[h]++;
          occ.emplace_back(srcs[i], (uint32_t)h);
          hadj_ptr[srcs[i] + 1]++;
        }
      if (hcnt[h] == 0) hcand.push_back((uint32_t)h);
    }
    for (size_t v = 0; v < nv; v++) hadj_ptr[v + 1] += hadj_ptr[v];
    hadj.resize(occ.size());
    std::vector<uint32_t> fill(hadj_ptr.begin(), hadj_ptr.end() - 1);
    for (const auto &o : occ) hadj[fill[o.first]++] = o.second;
    hs->kinds.clear();
    hs->n_wires = hs->n_run = 0;
  }
  std::vector<uint8_t> is_step(m, 0);
  std::vector<uint64_t> ksum(L);
  for (size_t j = 0; j < m; j++)
    if (candidate(j)) cand.push_back((uint32_t)j);
  P->rows.clear();
  P->wires.clear();
  P->level_ptr.assign(1, 0);
  k.clear();
  size_t n_constraint_steps = 0;
  for (uint32_t level = 1; !cand.empty() || !hcand.empty(); level++) {
    std::sort(cand.begin(), cand.end());  // a constraint becomes a candidate once: no duplicates
    fresh.clear();
    for (const uint32_t j : cand) {
      if (!candidate(j)) continue;  // its last unknown was determined in the level that made it a candidate
      uint32_t t = ~0u;
      for (uint32_t i = c_ptr[j]; i < c_ptr[j + 1]; i++)
        if (!known[c_list[i]]) t = c_list[i];
      if (claimed[t] == level) continue;  // a lower constraint of this level determines it
      if (n_hints && reserved[t]) continue;  // its hint determines it, or nothing does
      bool poly = false;
      std::fill(ksum.begin(), ksum.end(), 0);
      const size_t z = cs->nnz[2];
      for (uint32_t e = cs->h_row_ptr[2][j]; e < cs->h_row_ptr[2][j + 1]; e++) {
        if (cs->h_col[2][e] != t + 1) continue;
        if (!cs->h_pidx[2].empty() && cs->h_pidx[2][e] >= 0) poly = true;
        for (int l = 0; l < L; l++) ksum[l] = host::addmod(ksum[l], cs->h_coeff[2][(size_t)l * z + e], ctx->q[l]);
      }
      if (poly || std::find(ksum.begin(), ksum.end(), 0) != ksum.end()) continue;  // never ready as things stand
      claimed[t] = level;
      is_step[j] = 1;
      P->rows.push_back(j);
      P->wires.push_back(t);
      k.insert(k.end(), ksum.begin(), ksum.end());
      fresh.push_back(t);
    }
    n_constraint_steps += fresh.size();
    const size_t level_lo = P->rows.size() - fresh.size();
    if (n_hints) {
      hs->kinds.resize(P->rows.size(), 0);
      std::sort(hcand.begin(), hcand.end());  // a hint becomes ready once: no duplicates
      for (const uint32_t h : hcand) {
        hint_done[h] = 1;
        hs->n_run++;
        P->rows.push_back(h);
        P->wires.push_back(hints[h].dst);
        k.insert(k.end(), (size_t)L, 1);
        hs->kinds.push_back(1);
        for (size_t t = 0; t < targets(h); t++) fresh.push_back((uint32_t)(hints[h].dst + t * stride(h)));
      }
      hcand.clear();
    }
    if (fresh.empty()) break;
    P->level_ptr.push_back(P->rows.size());
    info.max_width = std::max<uint64_t>(info.max_width, P->rows.size() - level_lo);
    next.clear();
    for (const uint32_t t : fresh) known[t] = 1;
    for (const uint32_t t : fresh)
      for (uint32_t i = adj_ptr[t]; i < adj_ptr[t + 1]; i++) {
        const uint32_t j = adj[i] >> 1;
        (adj[i] & 1u ? cnt_c : cnt_ab)[j]--;
        if (candidate(j)) next.push_back(j);
      }
    if (n_hints)
      for (const uint32_t t : fresh)
        for (uint32_t i = hadj_ptr[t]; i < hadj_ptr[t + 1]; i++)
          if (--hcnt[hadj[i]] == 0) hcand.push_back(hadj[i]);
    cand.swap(next);
  }
  info.n_solved = n_constraint_steps;
  if (n_hints) {
    for (size_t h = 0; h < n_hints; h++)
      if (hint_done[h]) info.n_solved += targets(h);
    hs->n_wires = info.n_solved;
    hs->n_blocked = n_hints - hs->n_run;
    hs->first_blocked = std::find(hint_done.begin(), hint_done.end(), 0) - hint_done.begin();
  }
  info.n_unsolved = nv - info.n_given - info.n_solved;
  info.n_levels = P->level_ptr.size() - 1;
  info.n_unused = m - n_constraint_steps;
  info.first_unsolved = nv;
  for (size_t v = 0; v < nv; v++)
    if (!known[v]) {
      info.first_unsolved = v;
      break;
    }
  info.first_blocked = m;
  for (size_t j = 0; j < m; j++)
    if (!is_step[j] && cnt_ab[j] + cnt_c[j] > 0) {
      info.first_blocked = j;
      break;
    }
  if (info.first_blocked < m) {
    const size_t j = info.first_blocked;
    uint32_t in_ab = ~0u;  // the unknown of a and b when there is one only
    for (int w = 0; w < 2; w++)
      for (uint32_t e = cs->h_row_ptr[w][j]; e < cs->h_row_ptr[w][j + 1]; e++)
        if (cs->h_col[w][e] && !known[cs->h_col[w][e] - 1]) in_ab = cs->h_col[w][e] - 1;
    uint32_t t = ~0u;
    bool poly = false;
    for (uint32_t e = cs->h_row_ptr[2][j]; e < cs->h_row_ptr[2][j + 1]; e++)
      if (cs->h_col[2][e] && !known[cs->h_col[2][e] - 1]) {
        t = cs->h_col[2][e] - 1;
        if (!cs->h_pidx[2].empty() && cs->h_pidx[2][e] >= 0) poly = true;
      }
    if (cnt_c[j] == 1 && cnt_ab[j] == 1 && in_ab == t) info.blocked_reason = 5;
    else if (cnt_ab[j] > 0) info.blocked_reason = 1;
    else if (cnt_c[j] > 1) info.blocked_reason = 2;
    else if (n_hints && reserved[t]) info.blocked_reason = 6;
    else info.blocked_reason = poly ? 3 : 4;
  }
}

// algorithmic bytes of the steps [s_lo, s_hi): the distinct wires read or written times S * 8, plus the CSR entries and the
// schedule words touched; FP64 instructions per lane: a modular multiply-add per entry, the product and k^-1 per step
void launch_cost(const rs_ctx *ctx, const rs_r1cs_solve_plan *P, std::vector<uint32_t> &seen, uint32_t token, SolveLaunch &ln) {
  const rs_r1cs *cs = P->cs;
  double wires = 0, entries = 0;
  for (size_t s = ln.s_lo; s < ln.s_hi; s++) {
    const uint32_t j = P->rows[s];
    if (seen[P->wires[s] + 1] != token) seen[P->wires[s] + 1] = token, wires++;
    for (int w = 0; w < 3; w++)
      for (uint32_t e = cs->h_row_ptr[w][j]; e < cs->h_row_ptr[w][j + 1]; e++) {
        const uint32_t c = cs->h_col[w][e];
        entries++;
        if (c && seen[c] != token) seen[c] = token, wires++;
      }
  }
  const double S = (double)ctx->ring_words(), steps = (double)(ln.s_hi - ln.s_lo);
  ln.bytes = wires * S * 8 + entries * (4 + 8.0 * ctx->L) + steps * (8 + 6 * 4 + 8.0 * ctx->L);
  ln.ops = 7.0 * (entries + 2 * steps) * S;
}

static void build_launches(const rs_ctx *ctx, rs_r1cs_solve_plan *P) {
  const size_t n_levels = P->level_ptr.size() - 1, n_steps = P->rows.size();
  const size_t chunks = (ctx->ring_words() / 2 + 255) / 256;
  for (auto &l : P->launches) l.clear();
  if (n_steps == 0 || chunks == 0) return;
  for (size_t l = 0; l < n_levels; l++) P->launches[RS_SOLVE_LEVELS].push_back(SolveLaunch{0, P->level_ptr[l], P->level_ptr[l + 1], 0, 0});
  P->launches[RS_SOLVE_WALK].push_back(SolveLaunch{1, 0, n_steps, 0, 0});
  std::vector<SolveLaunch> &autol = P->launches[RS_SOLVE_AUTO];
  for (size_t l = 0; l < n_levels; l++) {
    const size_t lo = P->level_ptr[l], hi = P->level_ptr[l + 1];
    if ((hi - lo) * chunks >= SOLVE_FILL_WORKGROUPS) autol.push_back(SolveLaunch{0, lo, hi, 0, 0});
    else if (!autol.empty() && autol.back().kind == 1) autol.back().s_hi = hi;
    else autol.push_back(SolveLaunch{1, lo, hi, 0, 0});
  }
  std::vector<uint32_t> seen(P->cs->n_vars + 1, 0);
  uint32_t token = 0;
  for (auto &list : P->launches)
    for (SolveLaunch &ln : list) launch_cost(ctx, P, seen, ++token, ln);
}

template <class M>
static void solve_launch_arith(rs_ctx *ctx, const rs_r1cs_solve_plan *P, uint64_t *d_asg, const SolveLaunch &ln, hipStream_t st) {
  using T = typename ArithOf<M>::T;
  const rs_r1cs *cs = P->cs;
  SolveCsr<T> k;
  for (int w = 0; w < 3; w++) {
    k.rp[w] = cs->d_row_ptr[w];
    k.col[w] = cs->d_col[w];
    k.cf[w] = reinterpret_cast<const T *>(cs->d_coeff[w]);
    k.nnz[w] = cs->nnz[w];
    k.px[w] = cs->d_pidx[w];
  }
  k.ptab = reinterpret_cast<const T *>(cs->d_ptab);
  const T *kinv = reinterpret_cast<const T *>(P->d_kinv);
  const size_t n_steps = P->rows.size(), chunks = (ctx->ring_words() / 2 + 255) / 256;
  if (ln.kind == 0) {
    size_t spw = SOLVE_STEPS_PER_WG;
    while (spw > 1 && chunks * ((ln.s_hi - ln.s_lo + spw - 1) / spw) < 4096) spw >>= 1;
    const size_t groups = (ln.s_hi - ln.s_lo + spw - 1) / spw;
    RS_REQUIRE(chunks * groups < ((size_t)1 << 31), "level too wide for one launch of the solver");
    ProfScope p(ctx, st, "solve_level", ln.bytes, ln.ops);
    hipLaunchKernelGGL(solve_level_kernel<M>, dim3((unsigned)(chunks * groups)), dim3(256), 0, st, k, P->d_rows, P->d_wires, kinv, n_steps,
                       ln.s_lo, ln.s_hi, d_asg, ctx->N, ctx->L, CtxArith<M>::qmod(ctx), (unsigned)groups, (unsigned)spw);
  } else {
    ProfScope p(ctx, st, "solve_walk", ln.bytes, ln.ops);
    hipLaunchKernelGGL(solve_walk_kernel<M>, dim3((unsigned)chunks), dim3(256), 0, st, k, P->d_rows, P->d_wires, kinv, n_steps, ln.s_lo,
                       ln.s_hi, d_asg, ctx->N, ctx->L, CtxArith<M>::qmod(ctx));
  }
  RS_HIP(hipGetLastError());
}

void solve_launch(rs_ctx *ctx, const rs_r1cs_solve_plan *P, uint64_t *d_asg, const SolveLaunch &ln, hipStream_t st) {
  dispatch_arith(ctx, [&](auto tag) { solve_launch_arith<decltype(tag)>(ctx, P, d_asg, ln, st); });
}

template <class M>
static uint64_t konst_bits(uint64_t v, uint64_t p) {
  const typename HostArith<M>::T c = HostArith<M>::konst(v, p);
  uint64_t w;
  static_assert(sizeof(c) == sizeof(w), "constants of both arithmetics travel as 64-bit words");
  std::memcpy(&w, &c, sizeof(w));
  return w;
}

void upload_schedule(const rs_ctx *ctx, rs_r1cs_solve_plan *P, const std::vector<uint64_t> &k, const uint8_t *kinds, size_t n_index) {
  const rs_r1cs *cs = P->cs;
  // everything that indexes memory on the device, checked before any launch can use it
  const size_t n = P->rows.size(), L = (size_t)ctx->L;
  RS_REQUIRE(P->wires.size() == n && k.size() == n * L && P->level_ptr.front() == 0 && P->level_ptr.back() == n, "inconsistent schedule");
  for (size_t s = 0; s < n; s++)
    RS_REQUIRE(P->rows[s] < (kinds && kinds[s] ? n_index : cs->m) && P->wires[s] < cs->n_vars, "schedule index out of range");
  for (size_t l = 0; l + 1 < P->level_ptr.size(); l++) RS_REQUIRE(P->level_ptr[l] < P->level_ptr[l + 1], "level pointers are not monotone");
  if (!n) return;
  std::vector<uint64_t> kinv(L * n);
  for (size_t s = 0; s < n; s++)
    for (size_t l = 0; l < L; l++) {
      const uint64_t inv = host::invmod(k[s * L + l], ctx->q[l]);
      kinv[l * n + s] = ctx->use_int ? konst_bits<ModI>(inv, ctx->q[l]) : konst_bits<Mod>(inv, ctx->q[l]);
    }
  RS_HIP(hipMalloc(&P->d_rows, sizeof(uint32_t) * n));
  RS_HIP(hipMalloc(&P->d_wires, sizeof(uint32_t) * n));
  RS_HIP(hipMalloc(&P->d_kinv, sizeof(uint64_t) * L * n));
  RS_HIP(hipMemcpy(P->d_rows, P->rows.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  RS_HIP(hipMemcpy(P->d_wires, P->wires.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  RS_HIP(hipMemcpy(P->d_kinv, kinv.data(), sizeof(uint64_t) * L * n, hipMemcpyHostToDevice));
}

}  // namespace rs

using namespace rs;

extern "C" {

int rs_r1cs_solve_plan_create(rs_ctx *ctx, const rs_r1cs *cs, const uint8_t *h_given, rs_r1cs_solve_plan **out, rs_r1cs_solve_info *h_info) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(cs && out && (h_given || cs->n_vars == 0), "null argument");
  RS_REQUIRE(cs->L == ctx->L, "constraint system of another context");
  struct Holder {  // frees a partly built plan when a check below throws
    rs_r1cs_solve_plan *p;
    ~Holder() { rs_r1cs_solve_plan_destroy(p); }
  } holder{new rs_r1cs_solve_plan()};
  rs_r1cs_solve_plan *P = holder.p;
  P->ctx = ctx;
  P->cs = cs;
  std::vector<uint64_t> k;
  build_schedule(ctx, cs, h_given, P, k);
  upload_schedule(ctx, P, k);
  build_launches(ctx, P);
  if (h_info) *h_info = P->info;
  holder.p = nullptr;
  *out = P;
  RS_API_END
}

int rs_r1cs_solve_plan_steps(const rs_r1cs_solve_plan *plan, uint32_t *h_rows, uint32_t *h_wires, uint64_t *h_level_ptr) {
  RS_API_BEGIN
  RS_REQUIRE(plan, "null argument");
  if (h_rows) std::copy(plan->rows.begin(), plan->rows.end(), h_rows);
  if (h_wires) std::copy(plan->wires.begin(), plan->wires.end(), h_wires);
  if (h_level_ptr) std::copy(plan->level_ptr.begin(), plan->level_ptr.end(), h_level_ptr);
  RS_API_END
}

void rs_r1cs_solve_plan_destroy(rs_r1cs_solve_plan *plan) {
  if (!plan) return;
  if (plan->d_rows) (void)hipFree(plan->d_rows);
  if (plan->d_wires) (void)hipFree(plan->d_wires);
  if (plan->d_kinv) (void)hipFree(plan->d_kinv);
  delete plan;
}

int rs_r1cs_solve(rs_ctx *ctx, const rs_r1cs_solve_plan *plan, uint64_t *d_assignment, int mode, rs_r1cs_solve_stats *h_stats,
                  rs_stream stream) {
  RS_API_BEGIN_CTX(ctx)
  RS_REQUIRE(plan && d_assignment, "null argument");
  RS_REQUIRE(plan->ctx == ctx, "solve plan of another context");
  RS_REQUIRE(mode == RS_SOLVE_AUTO || mode == RS_SOLVE_LEVELS || mode == RS_SOLVE_WALK, "unknown solve mode");
  const std::vector<SolveLaunch> &launches = plan->launches[mode];
  rs_r1cs_solve_stats stats{0, 0};
  for (const SolveLaunch &ln : launches) (ln.kind == 0 ? stats.level_launches : stats.walk_launches)++;
  if (!launches.empty()) {
    std::unique_lock<std::mutex> lk(ctx->mu, std::defer_lock);
    if (ctx->profiling) lk.lock();  // the record ProfScope appends to belongs to the holder of mu
    for (const SolveLaunch &ln : launches) solve_launch(ctx, plan, d_assignment, ln, S(stream));
  }
  if (h_stats) *h_stats = stats;
  RS_API_END
}

}  // extern "C"
