// witness_plan.hip -- the witness map's per-(context, m) plan: host-side construction of the tables of witness_plan.hpp, the
// plan cache, and the column plans the kernels read them through.  Host code only: no kernel is defined or launched here
// (witness.hip has the map of the units).
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>

#include "witness_inc.hpp"
#include "witness_launch.hpp"

namespace rs {

// ---- host-side helpers (integer arithmetic; builds the tables above) -------------------------
namespace hostw {
using namespace host;

struct CycTab {
  uint64_t p;
  int logmax;                     // transforms up to length 2^logmax
  std::vector<uint64_t> tw, itw;  // tw[Mg + i] = w_{2Mg}^{bitrev(i)}
};
static CycTab make_cyc(uint64_t p, int logn_max) {
  CycTab t;
  t.p = p;
  t.logmax = logn_max;
  const size_t n = (size_t)1 << logn_max;
  t.tw.assign(n, 1);
  t.itw.assign(n, 1);
  const uint64_t wtop = some_primitive_root((uint64_t)n, p);  // primitive n-th root
  for (int lg = 0; (1u << lg) < n; lg++) {
    const size_t Mg = (size_t)1 << lg;  // groups
    // w_{2Mg} = wtop^(n / 2Mg)
    const uint64_t w2 = powmod(wtop, (uint64_t)(n / (2 * Mg)), p);
    std::vector<uint64_t> pw(Mg);
    uint64_t c = 1;
    for (size_t e = 0; e < Mg; e++) {
      pw[e] = c;
      c = mulmod(c, w2, p);
    }
    for (size_t i = 0; i < Mg; i++) {
      const uint64_t v = pw[bitrev((uint32_t)i, lg)];
      t.tw[Mg + i] = v;
      t.itw[Mg + i] = invmod(v, p);
    }
  }
  return t;
}
// nst >= 0: the first nst stages only (incomplete transforms, witness_inc.hpp: leaves of 2^(logn - nst) consecutive words)
static void ntt_fwd(std::vector<uint64_t> &a, int logn, const CycTab &t, int nst = -1) {
  const size_t n = (size_t)1 << logn;
  const uint64_t p = t.p;
  const size_t mend = nst < 0 ? n : (size_t)1 << nst;
  for (size_t m = 1, gap = n >> 1; m < mend; m <<= 1, gap >>= 1)
    for (size_t i = 0; i < m; i++) {
      const uint64_t W = t.tw[m + i];
      for (size_t j = 2 * i * gap; j < 2 * i * gap + gap; j++) {
        const uint64_t u = a[j], v = mulmod(a[j + gap], W, p);
        a[j] = addmod(u, v, p);
        a[j + gap] = submod(u, v, p);
      }
    }
}
// u0 > 0: the inverse of an incomplete transform -- stages u0 .. logn-1, scaled by 2^-(logn - u0)
static void ntt_inv(std::vector<uint64_t> &a, int logn, const CycTab &t, int u0 = 0) {
  const size_t n = (size_t)1 << logn;
  const uint64_t p = t.p;
  for (size_t m = n >> (u0 + 1), gap = (size_t)1 << u0; m >= 1; m >>= 1, gap <<= 1)
    for (size_t i = 0; i < m; i++) {
      const uint64_t W = t.itw[m + i];
      for (size_t j = 2 * i * gap; j < 2 * i * gap + gap; j++) {
        const uint64_t u = a[j], v = a[j + gap];
        a[j] = addmod(u, v, p);
        a[j + gap] = mulmod(submod(u, v, p), W, p);
      }
    }
  const uint64_t ninv = invmod((uint64_t)(n >> u0) % p, p);
  for (auto &x : a) x = mulmod(x, ninv, p);
}
static int clog2(size_t x) {
  int l = 0;
  while (((size_t)1 << l) < x) l++;
  return l;
}
static std::vector<uint64_t> polymul(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const CycTab &t) {
  const size_t need = a.size() + b.size() - 1;
  if (std::min(a.size(), b.size()) <= 16) {
    std::vector<uint64_t> o(need, 0);
    for (size_t i = 0; i < a.size(); i++)
      for (size_t j = 0; j < b.size(); j++) o[i + j] = addmod(o[i + j], mulmod(a[i], b[j], t.p), t.p);
    return o;
  }
  const int lg = clog2(need);
  if (lg > t.logmax && lg - t.logmax <= 4) {
    // the prime has no root of unity of that order: incomplete transforms (witness_inc.hpp) -- the first logmax stages, then
    // the product of the residues modulo x^G - eta per leaf, G = 2^(lg - logmax)
    const int inc = lg - t.logmax, nst = t.logmax;
    const size_t G = (size_t)1 << inc, n = (size_t)1 << lg;
    std::vector<uint64_t> fa(a), fb(b), out(n);
    fa.resize(n, 0);
    fb.resize(n, 0);
    ntt_fwd(fa, lg, t, nst);
    ntt_fwd(fb, lg, t, nst);
    for (size_t g = 0; g < (n >> inc); g++) {
      const uint64_t w = t.tw[(((size_t)1 << nst) + g) >> 1], eta = (g & 1) ? (t.p - w) % t.p : w;
      const uint64_t *x = &fa[g * G], *y = &fb[g * G];
      for (size_t k = 0; k < G; k++) {
        uint64_t lo = 0, hi = 0;
        for (size_t i = 0; i < G; i++) {
          const uint64_t pr = mulmod(x[i], y[(k - i) & (G - 1)], t.p);
          if (i <= k) lo = addmod(lo, pr, t.p);
          else hi = addmod(hi, pr, t.p);
        }
        out[g * G + k] = addmod(lo, mulmod(hi, eta, t.p), t.p);
      }
    }
    ntt_inv(out, lg, t, inc);
    out.resize(need);
    return out;
  }
  if (lg > t.logmax) {
    // ... more than four stages short: block convolution over blocks of Bh = 2^(logmax-1)
    // coefficients (each block product fits one transform of length 2 Bh), overlap-added
    const size_t Bh = (size_t)1 << (t.logmax - 1);
    const size_t nab = (a.size() + Bh - 1) / Bh, nbb = (b.size() + Bh - 1) / Bh;
    auto spectra = [&](const std::vector<uint64_t> &x, size_t nb) {
      std::vector<std::vector<uint64_t>> sp(nb);
      for (size_t i = 0; i < nb; i++) {
        sp[i].assign(2 * Bh, 0);
        for (size_t k = 0; k < Bh && i * Bh + k < x.size(); k++) sp[i][k] = x[i * Bh + k];
        ntt_fwd(sp[i], t.logmax, t);
      }
      return sp;
    };
    const auto sa = spectra(a, nab), sb = spectra(b, nbb);
    std::vector<uint64_t> o(need + 2 * Bh, 0);
    for (size_t k = 0; k + 1 < nab + nbb; k++) {
      std::vector<uint64_t> acc(2 * Bh, 0);
      for (size_t i = (k >= nbb ? k - nbb + 1 : 0); i <= k && i < nab; i++)
        for (size_t x = 0; x < 2 * Bh; x++) acc[x] = addmod(acc[x], mulmod(sa[i][x], sb[k - i][x], t.p), t.p);
      ntt_inv(acc, t.logmax, t);
      for (size_t x = 0; x < 2 * Bh; x++) o[k * Bh + x] = addmod(o[k * Bh + x], acc[x], t.p);
    }
    o.resize(need);
    return o;
  }
  std::vector<uint64_t> fa(a), fb(b);
  fa.resize((size_t)1 << lg, 0);
  fb.resize((size_t)1 << lg, 0);
  ntt_fwd(fa, lg, t);
  ntt_fwd(fb, lg, t);
  for (size_t i = 0; i < fa.size(); i++) fa[i] = mulmod(fa[i], fb[i], t.p);
  ntt_inv(fa, lg, t);
  fa.resize(need);
  return fa;
}
}  // namespace hostw

static void *up(const std::vector<uint64_t> &h) {
  void *d = nullptr;
  RS_HIP(hipMalloc(&d, std::max<size_t>(1, h.size()) * sizeof(uint64_t)));
  if (!h.empty()) RS_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  return d;
}
// the 8-byte word of a table constant / of a data value in the context's arithmetic
static uint64_t word_of(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}
static uint64_t word_of(uint64_t u) { return u; }
uint64_t konst_word(const rs_ctx *ctx, uint64_t v, uint64_t p) {
  return ctx->use_int ? word_of(HostArith<ModI>::konst(v, p)) : word_of(HostArith<Mod>::konst(v, p));
}
static uint64_t plain_word(const rs_ctx *ctx, uint64_t v, uint64_t p) {
  return ctx->use_int ? word_of(HostArith<ModI>::plain(v, p)) : word_of(HostArith<Mod>::plain(v, p));
}

// largest tile of the product tree in the multi-pass path: full transforms of that length run inside the tile kernels
static int tree_tile_log(bool fp, int logM) {
  const int logT = std::min(g_tune.witness_lds_logM, logM);
  return (fp && logT == 13 && logM >= 15 && g_tune.witness_tree_ct == 2 && g_tune.witness_tree_log >= 14) ? 14 : logT;
}

static void free_plan_tables(WitnessPlan *P);
static WitnessPlan *build_plan(rs_ctx *ctx, size_t m) {
  using namespace hostw;
  RS_REQUIRE(m >= 1, "need at least one constraint");
  WitnessPlan *P = new WitnessPlan();
  P->m = m;
  P->logM = std::max(1, clog2(m));
  P->M = (size_t)1 << P->logM;
  const size_t M = P->M;
  const int logM = P->logM;
  if (logM > 22)
    throw Error(RS_ERR_UNSUPPORTED, "witness map beyond 2^22 constraints is not supported");
  P->limb.resize(ctx->L);
  int vmin = 64;
  for (int li = 0; li < ctx->L; li++) vmin = std::min(vmin, host::two_adicity(ctx->q[li]));
  if (g_tune.witness_force_bc > 0) vmin = std::min(vmin, g_tune.witness_force_bc);  // tests: the block path on well-endowed primes
  const bool blocked = vmin < logM + 1;
  // Incomplete transforms (witness_inc.hpp): the multi-pass path as it is, every transform longer than 2^(a prime's
  // 2-adicity) stopped that many stages early.  Needs: columns that take the multi-pass path; full transforms inside the
  // product tree's tiles; at most RS_INC_MAX stages missing, all of them inside the LAST round of a sub-transform block.
  {
    const int logT = std::min(g_tune.witness_lds_logM, logM);
    // (M = 2^14 on the FP64 arithmetic normally runs in ONE 2^14 tile -- single_tile_ok -- whose Newton conversion needs a
    // complete 2^15-point transform: a prime without it takes the multi-pass path on 2^13 tiles instead, one stage short)
    const bool multi = logM > g_tune.witness_lds_logM;
    P->incomplete = blocked && g_tune.witness_inc && multi && vmin >= tree_tile_log(!ctx->use_int, logM) && logM + 1 - vmin <= RS_INC_MAX &&
                    std::min(logT, 12) > RS_INC_MAX;
  }
  const bool bcpath = blocked && !P->incomplete;
  // full-length transforms serve 2^21 and 2^22 constraints as they serve 2^20 (one more cross pass), complete or not; the
  // block convolutions stop at 2^20 (the two-level transform across blocks is built for Y <= 256 blocks of 2^13)
  if (bcpath && logM > 20)
    throw Error(RS_ERR_UNSUPPORTED, "witness map beyond 2^20 constraints needs ring primes = 1 mod 2^(log2 M - 3) (full-length transforms, "
                                    "at most four stages short); the block convolutions of other primes stop at 2^20");
  P->bc2 = bcpath && g_tune.witness_bc2 && !ctx->use_int && vmin >= 14 && logM >= 15;
  P->bcLog = bcpath ? (P->bc2 ? 14 : std::min(vmin, 13)) : 0;
  // every context prime is 1 mod 2*N_enc with N_enc >= 16, so the 2-adicity is at least 5
  RS_REQUIRE(!bcpath || P->bcLog > SCHOOL_LEVELS, "ring prime with too little 2-adicity for the witness map");
  const size_t Bc = bcpath ? (size_t)1 << (P->bcLog - 1) : 0, nblk = bcpath ? std::max<size_t>(1, M / Bc) : 0;
  // one host thread per ring limb: the tables of different primes are independent (product tree, Newton iteration for
  // rev(Z)^-1 -- 0.6 s per limb at the headline, the bulk of a process's first proof)
  auto build_limb = [&](int li) {
    LimbPlan &lp = P->limb[li];
    const uint64_t p = ctx->q[li];
    RS_REQUIRE(p > 2 * M, "ring prime too small for the evaluation domain");
    lp.p = p;
    // longest transform the device tables serve: the block length (block convolutions), this prime's 2-adicity
    // (incomplete transforms: longer ones stop there), else 2M
    lp.adic = 64;
    if (P->incomplete) {
      int a = host::two_adicity(p);
      if (g_tune.witness_force_bc > 0) a = std::min(a, g_tune.witness_force_bc);
      if (a < logM + 1) lp.adic = a;
    }
    const int tabLog = bcpath ? P->bcLog : std::min(logM + 1, lp.adic);
    auto inc_of = [&](int logn) { return logn > lp.adic ? logn - lp.adic : 0; };
    const CycTab T = make_cyc(p, tabLog);
    auto bal = [&](uint64_t v) { return konst_word(ctx, v, p); };
    {
      const size_t tn = (size_t)1 << tabLog;
      std::vector<uint64_t> tw(tn), itw(tn);
      for (size_t k = 0; k < tn; k++) tw[k] = bal(T.tw[k]), itw[k] = bal(T.itw[k]);
      lp.d_tw = up(tw);
      lp.d_itw = up(itw);
    }
    // spectra (scaled by 1/(2 Bc)) of the Bc-coefficient blocks of a polynomial: [blocks][2 Bc]
    auto block_spectra = [&](const std::vector<uint64_t> &poly, size_t blocks, bool raw = false) {
      std::vector<uint64_t> out(blocks * 2 * Bc, 0);
      const uint64_t sc = invmod((uint64_t)(2 * Bc) % p, p);
      for (size_t b = 0; b < blocks; b++) {
        std::vector<uint64_t> f(2 * Bc, 0);
        for (size_t k = 0; k < Bc && b * Bc + k < poly.size(); k++) f[k] = poly[b * Bc + k];
        ntt_fwd(f, P->bcLog, T);
        for (size_t k = 0; k < 2 * Bc; k++) out[b * 2 * Bc + k] = raw ? mulmod(f[k], sc, p) : bal(mulmod(f[k], sc, p));
      }
      return out;
    };
    // bc2: the Y-point transform across the (zero-padded) blocks of such spectra, point by point, scaled by 1/Y; output
    // [Y][2 Bc] in the order the device's forward transform across blocks leaves its results (host ntt_fwd order)
    auto across_blocks = [&](const std::vector<uint64_t> &poly, size_t blocks, uint64_t *dst) {
      const std::vector<uint64_t> sp = block_spectra(poly, blocks, true);
      const size_t Y = 2 * blocks;
      const int logY = clog2(Y);
      const uint64_t sc = invmod((uint64_t)Y % p, p);
      std::vector<uint64_t> v(Y);
      for (size_t k = 0; k < 2 * Bc; k++) {
        for (size_t y = 0; y < Y; y++) v[y] = y < blocks ? sp[y * 2 * Bc + k] : 0;
        ntt_fwd(v, logY, T);
        for (size_t y = 0; y < Y; y++) dst[y * 2 * Bc + k] = bal(mulmod(v[y], sc, p));
      }
    };
    lp.fwd_mask2 = fwd_reduce_mask(p, logM + 1);
    lp.inv_mask2 = inv_reduce_mask(p, logM + 1);
    // factorials
    std::vector<uint64_t> fact(M), ifact(M);
    fact[0] = 1;
    for (size_t j = 1; j < M; j++) fact[j] = mulmod(fact[j - 1], (uint64_t)j % p, p);
    ifact[M - 1] = invmod(fact[M - 1], p);
    for (size_t j = M - 1; j > 0; j--) ifact[j - 1] = mulmod(ifact[j], (uint64_t)j % p, p);
    {
      std::vector<uint64_t> v(M, 0);
      for (size_t j = 0; j < m; j++) v[j] = bal(ifact[j]);
      lp.d_invfact = up(v);
      std::vector<uint64_t> e(2 * M, 0);
      for (size_t k = 0; k < m; k++) e[k] = (k & 1) ? (p - ifact[k]) % p : ifact[k];
      if (bcpath) {
        e.resize(M);
        lp.d_bc_e = up(block_spectra(e, nblk));
        if (P->bc2) {
          std::vector<uint64_t> t2(2 * nblk * 2 * Bc);
          across_blocks(e, nblk, t2.data());
          lp.d_b2_e = up(t2);
        }
      } else {
        const int nst = logM + 1 - inc_of(logM + 1);  // the inverse undoes nst stages: scale 2^-nst
        ntt_fwd(e, logM + 1, T, nst);
        const uint64_t s2 = invmod(((uint64_t)1 << nst) % p, p);
        std::vector<uint64_t> eh(2 * M);
        for (size_t k = 0; k < 2 * M; k++) eh[k] = bal(mulmod(e[k], s2, p));
        lp.d_ehat = up(eh);
      }
    }
    // subproduct tree: prod[l][i] = prod_{j in [i 2^l, (i+1) 2^l)} (x - j), low 2^l coefficients
    std::vector<std::vector<std::vector<uint64_t>>> prod(logM + 1);
    prod[0].resize(M);
    for (size_t i = 0; i < M; i++) prod[0][i] = {(p - (uint64_t)i % p) % p};
    for (int l = 1; l <= logM; l++) {
      const size_t h = (size_t)1 << (l - 1);
      prod[l].resize(M >> l);
      for (size_t i = 0; i < (M >> l); i++) {
        const auto &a = prod[l - 1][2 * i], &b = prod[l - 1][2 * i + 1];
        std::vector<uint64_t> ab = polymul(a, b, T);  // degree <= 2h-2
        std::vector<uint64_t> r(2 * h, 0);
        for (size_t k = 0; k < ab.size(); k++) r[k] = ab[k];
        for (size_t k = 0; k < h; k++) r[h + k] = addmod(r[h + k], addmod(a[k], b[k], p), p);
        prod[l][i] = r;
      }
    }
    // D_left spectra (levels > SCHOOL_LEVELS) and low coefficients (levels <= SCHOOL_LEVELS)
    {
      std::vector<uint64_t> dhat((size_t)(logM + 1) * M, 0), dlow((size_t)(SCHOOL_LEVELS + 1) * (M / 2 + 1), 0);
      std::vector<uint64_t> bcd(bcpath && logM > P->bcLog ? (size_t)(logM - P->bcLog) * M : 0, 0);
      std::vector<uint64_t> b2d(P->bc2 && logM > P->bcLog ? (size_t)(logM - P->bcLog) * 2 * M : 0, 0);
      for (int l = 1; l <= logM; l++) {
        const size_t n = (size_t)1 << l, h = n >> 1;
        for (size_t i = 0; i < (M >> l); i++) {
          const auto &dl = prod[l - 1][2 * i];  // h low coefficients, monic of degree h
          if (l <= SCHOOL_LEVELS) {
            for (size_t k = 0; k < h; k++) dlow[(size_t)l * (M / 2 + 1) + i * h + k] = bal(dl[k]);
          } else if (bcpath && l > P->bcLog) {
            // node i of level l: the h / Bc blocks of D_left's low part (the monic x^h term is added by the sink)
            const std::vector<uint64_t> sp = block_spectra(dl, h / Bc);
            std::copy(sp.begin(), sp.end(), bcd.begin() + (size_t)(l - P->bcLog - 1) * M + i * n);
            if (P->bc2) across_blocks(dl, h / Bc, b2d.data() + (size_t)(l - P->bcLog - 1) * 2 * M + i * 2 * n);
          } else {
            std::vector<uint64_t> f(n, 0);
            for (size_t k = 0; k < h; k++) f[k] = dl[k];
            f[h] = 1;
            const int nst = l - inc_of(l);
            ntt_fwd(f, l, T, nst);
            const uint64_t sc = invmod(((uint64_t)1 << nst) % p, p);
            for (size_t k = 0; k < n; k++) dhat[(size_t)l * M + i * n + k] = bal(mulmod(f[k], sc, p));
          }
        }
      }
      // PRECONDITION of the kernels that skip the reduction before the table product (ColPlan::pwmask, fwd_end_needs_reduce in
      // rs_core.hip; tree_wide_kernel, sub_ntt_wide_kernel MODE 2): the spectrum may be as large as 2^50, so mulmod's
      // |a b| <= p 2^49 holds only for BALANCED table entries, |s| <= p/2.  Every entry goes through bal(); checked here so
      // that a future table built any other way fails at plan time, not as a wrong residue.
      if (!ctx->use_int) {
        auto balanced_table = [&](const std::vector<uint64_t> &t) {
          for (uint64_t wd : t) {
            double d;
            memcpy(&d, &wd, 8);
            if (!(d <= 0.5 * (double)p && d >= -0.5 * (double)p)) return false;
          }
          return true;
        };
        RS_REQUIRE(balanced_table(dhat) && balanced_table(bcd) && balanced_table(b2d), "internal: a spectrum table is not balanced (|s| <= p/2)");
      }
      lp.d_dhat = up(dhat);
      lp.d_dlow = up(dlow);
      if (!bcd.empty()) lp.d_bc_d = up(bcd);
      if (!b2d.empty()) lp.d_b2_d = up(b2d);
    }
    // Z = prod_{j<m} (x - j): product of the maximal aligned blocks of [0, m)
    {
      std::vector<uint64_t> Z = {1};
      size_t start = 0;
      for (int l = logM; l >= 0; l--) {
        const size_t len = (size_t)1 << l;
        if (start + len <= m) {
          std::vector<uint64_t> blk = prod[l][start >> l];
          blk.push_back(1);
          Z = polymul(Z, blk, T);
          start += len;
        }
      }
      RS_REQUIRE(Z.size() == m + 1 && start == m, "internal: vanishing polynomial size");
      lp.Z = Z;
      std::vector<uint64_t> zt(M, 0);
      for (size_t k = 0; k < M && k <= m; k++) zt[k] = bal(Z[k]);
      lp.d_ztab = up(zt);
      if (!blocked && M >= 2) {
        // H on a coset (Rinocchio, where C is interpolated anyway): H(g w^i) = (A B - C)(g w^i) / Z(g w^i) at the M points
        // g w^i, none of which may be a root of Z (an integer 0 .. m-1; the point g w^0 = g itself is one for g < m): try
        // g = m + 1, m + 2, ... until Z has no zero there (a given g fails with probability ~ m M / q)
        const uint64_t mi = invmod((uint64_t)M % p, p);
        for (uint64_t g = (uint64_t)m + 1;; g++) {
          RS_REQUIRE(g < (uint64_t)m + 1000, "internal: no coset for the vanishing polynomial");
          std::vector<uint64_t> gp(M), zc(M, 0);
          gp[0] = 1;
          for (size_t k = 1; k < M; k++) gp[k] = mulmod(gp[k - 1], g % p, p);
          for (size_t k = 0; k < M && k <= m; k++) zc[k] = mulmod(Z[k], gp[k], p);
          if (m == M) zc[0] = addmod(zc[0], mulmod(gp[M - 1], g % p, p), p);  // x^M = g^M on the coset
          ntt_fwd(zc, logM, T);
          bool ok = true;
          for (size_t k = 0; k < M && ok; k++) ok = zc[k] != 0;
          if (!ok) continue;
          // batch inversion of the M values
          std::vector<uint64_t> pre(M);
          uint64_t acc = 1;
          for (size_t k = 0; k < M; k++) {
            pre[k] = acc;
            acc = mulmod(acc, zc[k], p);
          }
          uint64_t inv = invmod(acc, p);
          std::vector<uint64_t> zi(M), gh(M), gg(M);
          for (size_t k = M; k-- > 0;) {
            zi[k] = bal(mulmod(inv, pre[k], p));
            inv = mulmod(inv, zc[k], p);
          }
          const uint64_t ginv = invmod(g % p, p);
          uint64_t gi = mi;  // g^-k / M
          for (size_t k = 0; k < M; k++) {
            gg[k] = bal(gp[k]);
            gh[k] = bal(gi);
            gi = mulmod(gi, ginv, p);
          }
          lp.d_cos_g = up(gg);
          lp.d_cos_h = up(gh);
          lp.d_cos_z = up(zi);
          break;
        }
      }
      // S = rev(Z)^-1 mod x^(m-1) (Newton iteration): quo(P, Z) = rev(rev(P) * S mod x^(m-1)) for
      // deg P = 2m-2.  Spectrum at length 2M, scaled by 1/(2M)^2 (two unscaled inverse transforms).
      std::vector<uint64_t> shat(2 * M, 0);
      if (m >= 2) {
        std::vector<uint64_t> f(m - 1);
        for (size_t i2 = 0; i2 + 1 < m; i2++) f[i2] = Z[m - i2];  // rev(Z), constant term Z[m] = 1
        std::vector<uint64_t> g = {1};
        while (g.size() < m - 1) {
          const size_t k2 = std::min(2 * g.size(), m - 1);
          std::vector<uint64_t> fk(f.begin(), f.begin() + k2);
          std::vector<uint64_t> fg = polymul(fk, g, T);
          fg.resize(k2);
          for (auto &x : fg) x = (p - x) % p;  // -f*g
          fg[0] = addmod(fg[0], 2, p);         // 2 - f*g
          std::vector<uint64_t> ng = polymul(g, fg, T);
          ng.resize(k2);
          g = ng;
        }
        for (size_t i2 = 0; i2 < g.size(); i2++) shat[i2] = g[i2];
        if (!bcpath) {
          const int nst = logM + 1 - inc_of(logM + 1);
          ntt_fwd(shat, logM + 1, T, nst);
          const uint64_t s2 = invmod(((uint64_t)1 << nst) % p, p), s4 = mulmod(s2, s2, p);
          for (auto &x : shat) x = mulmod(x, s4, p);
        }
      }
      if (bcpath) {
        shat.resize(M);  // S itself, m - 1 <= M coefficients
        lp.d_bc_s = up(block_spectra(shat, nblk));
        if (P->bc2) {
          std::vector<uint64_t> t2(2 * nblk * 2 * Bc);
          across_blocks(shat, nblk, t2.data());
          lp.d_b2_s = up(t2);
        }
      } else {
        std::vector<uint64_t> sh(2 * M);
        for (size_t k = 0; k < 2 * M; k++) sh[k] = bal(shat[k]);
        lp.d_shat = up(sh);
      }
    }
  };
  {
    std::vector<std::thread> workers;
    std::vector<std::string> errs(ctx->L);
    std::vector<int> codes(ctx->L, RS_OK);
    for (int li = 0; li < ctx->L; li++)
      workers.emplace_back([&, li] {
        try {
          RS_HIP(hipSetDevice(ctx->device));  // a new thread starts on device 0
          build_limb(li);
        } catch (const Error &e) {
          codes[li] = e.code;
          errs[li] = e.what();
        } catch (const std::exception &e) {
          codes[li] = RS_ERR_INVALID;
          errs[li] = e.what();
        }
      });
    for (auto &w : workers) w.join();
    for (int li = 0; li < ctx->L; li++)
      if (codes[li] != RS_OK) {
        free_plan_tables(P);
        delete P;
        throw Error(codes[li], errs[li]);
      }
  }
  return P;
}

static void free_plan_tables(WitnessPlan *P) {
  for (auto &lp : P->limb) {
    void *ptrs[] = {lp.d_tw, lp.d_itw, lp.d_invfact, lp.d_ehat, lp.d_dhat, lp.d_dlow, lp.d_shat, lp.d_ztab, lp.d_bc_e, lp.d_bc_s, lp.d_bc_d,
                    lp.d_b2_e, lp.d_b2_s, lp.d_b2_d, lp.d_cos_g, lp.d_cos_h, lp.d_cos_z};
    for (void *q : ptrs)
      if (q) (void)hipFree(q);
  }
}
static void free_plan(WitnessPlan *P) {
  free_plan_tables(P);
  if (P->d_Zt) (void)hipFree(P->d_Zt);
  delete P;
}

// the knobs build_plan's choice of path (full length / incomplete / block convolutions) and table forms depend on
static uint64_t plan_knob_sig() {
  uint64_t h = 1469598103934665603ull;
  for (int v : {g_tune.witness_lds_logM, g_tune.witness_tree_log, g_tune.witness_tree_ct, g_tune.witness_inc, g_tune.witness_bc2, g_tune.witness_force_bc})
    h = (h ^ (uint64_t)(uint32_t)v) * 1099511628211ull;
  return h;
}
// Plans are cached per (m, plan_knob_sig()) and live until witness_plans_destroy: a plan is never freed under a call
// that holds its tables, and no lookup synchronises.  Cost: a context on which plan-shaping knobs are flipped (tests and
// tools/ only; the product never changes a knob) keeps one plan per distinct signature it has seen.
WitnessPlan *get_plan(rs_ctx *ctx, size_t m) {
  const std::pair<size_t, uint64_t> key{m, plan_knob_sig()};
  auto it = ctx->plans.find(key);
  if (it != ctx->plans.end()) return it->second;
  return ctx->plans[key] = build_plan(ctx, m);
}

// Z as the provers hand it to the inner products: [m + 1][L] values on the device, built at first use (one blocking
// upload per plan; every later proof reads the cached array -- no host transpose, no synchronisation inside a proof)
const uint64_t *witness_Z_rows(rs_ctx *ctx, size_t m) {
  WitnessPlan *P = get_plan(ctx, m);
  if (!P->d_Zt) {
    const int L = ctx->L;
    std::vector<uint64_t> zt((size_t)L * (m + 1));
    for (int i = 0; i < L; i++)
      for (size_t t = 0; t <= m; t++) zt[t * L + i] = P->limb[i].Z[t];
    RS_HIP(hipMalloc(&P->d_Zt, zt.size() * sizeof(uint64_t)));
    RS_HIP(hipMemcpy(P->d_Zt, zt.data(), zt.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  return P->d_Zt;
}

// Column plans of limbs limb0, limb0+1, ...: entry k serves the k-th limb of a chunk
template <class M>
ColPlansT<M> make_colplans(rs_ctx *ctx, const WitnessPlan *P, int limb0) {
  using T = typename ArithOf<M>::T;
  ColPlansT<M> cp;
  memset(&cp, 0, sizeof(cp));
  for (int i = limb0; i < ctx->L; i++) {
    const LimbPlan &lp = P->limb[i];
    ColPlanT<M> &c = cp.l[i - limb0];
    c.mod = HostArith<M>::make(lp.p);
    c.tw = static_cast<const T *>(lp.d_tw);
    c.itw = static_cast<const T *>(lp.d_itw);
    c.invfact = static_cast<const T *>(lp.d_invfact);
    c.ehat = static_cast<const T *>(lp.d_ehat);
    c.dhat = static_cast<const T *>(lp.d_dhat);
    c.dlow = static_cast<const T *>(lp.d_dlow);
    c.shat = static_cast<const T *>(lp.d_shat);
    c.ztab = static_cast<const T *>(lp.d_ztab);
    c.bc_e = static_cast<const T *>(lp.d_bc_e);
    c.bc_s = static_cast<const T *>(lp.d_bc_s);
    c.bc_d = static_cast<const T *>(lp.d_bc_d);
    c.b2_e = static_cast<const T *>(lp.d_b2_e);
    c.b2_s = static_cast<const T *>(lp.d_b2_s);
    c.b2_d = static_cast<const T *>(lp.d_b2_d);
    c.cos_g = static_cast<const T *>(lp.d_cos_g);
    c.cos_h = static_cast<const T *>(lp.d_cos_h);
    c.cos_z = static_cast<const T *>(lp.d_cos_z);
    c.bc_inv2b = P->bcLog ? HostArith<M>::konst(host::invmod(((uint64_t)1 << P->bcLog) % lp.p, lp.p), lp.p) : T(0);
    c.b2_inv = P->bc2 ? HostArith<M>::konst(host::invmod((uint64_t)(4 * P->M) % lp.p, lp.p), lp.p) : T(0);
    c.fwd_mask2 = lp.fwd_mask2;
    c.inv_mask2 = lp.inv_mask2;
    c.pwmask = 0;
    c.adic = lp.adic;
    for (int l = 0; l < 24; l++) {
      c.fmask[l] = fwd_reduce_mask(lp.p, l);
      // an incomplete transform's inverse starts at stage inc(l) on reduced values (inc_polymul)
      c.imask[l] = inv_reduce_mask(lp.p, l, c.inc(l));
      if (fwd_end_needs_reduce(lp.p, l)) c.pwmask |= 1u << l;
    }
  }
  return cp;
}
template ColPlansT<Mod> make_colplans<Mod>(rs_ctx *, const WitnessPlan *, int);
template ColPlansT<ModI> make_colplans<ModI>(rs_ctx *, const WitnessPlan *, int);

// Columns handled by the M-tile kernels (fused Newton + tree, h_tile): 2^10 .. 2^13 at two workgroups
// per CU, and 2^14 (a 136 KiB tile, one 1024-thread workgroup per CU) when the tile knob is at its
// natural setting -- one launch instead of the multi-pass path.
bool single_tile_ok(int logM) {
  if (logM < 10) return false;
  return logM <= g_tune.witness_lds_logM || (logM == 14 && g_tune.witness_lds_logM == 13);
}

void witness_plans_destroy(rs_ctx *ctx) {
  for (auto &kv : ctx->plans) free_plan(kv.second);
  ctx->plans.clear();
}

}  // namespace rs
