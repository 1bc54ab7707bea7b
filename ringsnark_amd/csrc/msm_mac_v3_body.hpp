// msm_mac_v3_body.hpp -- the BODY of mac_kernel_v3 and mac_kernel_v3g (msm_mac.hpp), included once inside each of them: the two
// kernels differ in their argument structure `a` only (MacArgs3: two groups; MacArgs3G: six), and the text is shared as
// text -- not as a function template that both call -- so that the two-group kernel is compiled from the very tokens it
// always had and keeps its code.  In scope: template <bool PAIRED, int LOGN>, a, L, K, coeff_tabs.  No include guard.
  constexpr int n = 1 << LOGN, H = 4096, LOGP = LOGN - 12, PARTS = 1 << LOGP;
  static_assert(LOGN == 13 || (LOGN == 14 && !PAIRED), "half spectrum at 8192 points, quarter spectrum at 16384");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *s = reinterpret_cast<double *>(smem);
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  // block -> XCD slot x (blocks go to XCDs round-robin) and a position q in that XCD's sequence.  The 2K workgroups
  // that read one plaintext row (both halves of every prime) and the groups that read the same ciphertext words are
  // consecutive in ONE XCD's sequence: one of them fetches from memory, the others hit that XCD's L2.
  const unsigned b = blockIdx.x, x = b & 7u;
  unsigned q = b >> 3;
  const int g = (int)(q % (unsigned)a.n_groups);
  q /= (unsigned)a.n_groups;
  const unsigned hj = q % ((unsigned)PARTS * (unsigned)K);
  const unsigned rr = (q / ((unsigned)PARTS * (unsigned)K)) * 8u + x;  // (chunk, limb)
  const int h = (int)(hj & (unsigned)(PARTS - 1)), j = (int)(hj >> LOGP);
  const int limb = (int)(rr % (unsigned)L), chunk = (int)(rr / (unsigned)L);
  if (chunk >= a.n_chunks) return;
  const Mod mod = coeff_tabs[j].mod;
  const double *__restrict__ tw = coeff_tabs[j].d_tw;
  const uint32_t red_mask = a.red_mask[j];
  const int root = PARTS + h;
  // per-lane twiddles of rounds 2 and 3, fixed for the whole chunk
  const int lo = t & 15, hi = t >> 4;
  // round-2 twiddles tw[(root << (4+k)) + (hi << k) + b] (16 lanes share each) come from an LDS copy of the table's
  // first 1024 entries; the round-3 twiddles are the lane's own and stay in registers
  double *twl = s + 2 * (H + H / 16);
  for (int i = t; i < 1024; i += 256) twl[i] = tw[i];
  __syncthreads();
  double tw3[15];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int bk = 0; bk < (1 << k); bk++) tw3[(1 << k) - 1 + bk] = tw[(root << (8 + k)) + (t << k) + bk];
#pragma unroll
  for (int i = 0; i < 15; i++) pin(tw3[i]);
  // wave-uniform twiddles of stage 0 and round 1, as scalar registers: fetched through the table pointer inside the
  // term loop they would be vector loads, and waiting for the youngest vector load drains the ciphertext stream
  // twiddles of the folded stages, with the sign of this workgroup's half: x + w y for the low half, x - w y for the high
  const double w0 = uniform_f64(tw[1]);
  const double w1 = uniform_f64(tw[2 + (h >> 1)]);  // LOGN = 14: stage 1 of this quarter's half
  const double w0s = (LOGN == 13 ? (h & 1) : (h & 2)) ? -w0 : w0, w1s = (h & 1) ? -w1 : w1;
  double tw1[15];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int bk = 0; bk < (1 << k); bk++) tw1[(1 << k) - 1 + bk] = uniform_f64(tw[(root << k) + bk]);
  const size_t enc_words = (size_t)L * 2 * K * n;
  const size_t slab = (((size_t)limb * 2) * K + j) * (size_t)n + (size_t)h * H;  // component 0; component 1 is + K*n
  const size_t comp = (size_t)K * n;
  uint64_t *part = a.partial[g] + (size_t)chunk * a.part_stride + slab;
  const int r0 = wave * 1024;  // the wave's range of the half spectrum: 64 round-3 groups
  double acc[2][16];
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int i = 0; i < 8; i++) {
      acc[c][2 * i] = acc[c][2 * i + 1] = 0.0;
      if (a.accumulate) {
        const u64x2 v = reinterpret_cast<const u64x2 *>(part + c * comp + r0)[lane + 64 * i];
        acc[c][2 * i] = from_u64(v.x);
        acc[c][2 * i + 1] = from_u64(v.y);
      }
    }
  const unsigned long long tbeg = (unsigned long long)chunk * a.terms_per_chunk;
  const unsigned long long tend = min(tbeg + (unsigned long long)a.terms_per_chunk, a.terms[g]);
  const double *crow = a.C[g] + ((size_t)tbeg * L + limb) * (size_t)n + (PAIRED ? 2 * t : t);
  const uint64_t *ctp = a.crs + (size_t)tbeg * enc_words + slab + r0;
  double cl[16], ch[16];
  // The row in two batches of 32 registers, the first requested before the previous term's multiply-accumulate and
  // the second after it (all 64 at once do not fit beside it).  Paired rows (plain_center_wide_kernel): one 16-byte
  // load brings x[n'] and x[n' + 4096]; plain rows: the multiplied operands x[n' + 4096] first.
  auto load_row_a = [&]() {
#pragma unroll
    for (int e = 0; e < 16; e++) {
#if RS_MAC3_ABLATE & 1  // experiment: no plaintext-row traffic (wrong results)
      if (PAIRED ? e < 8 : true) ch[e] = 5.0 + t;
      if (PAIRED && e < 8) cl[e] = 3.0 + e;
#else
      if (PAIRED) {
        if (e < 8) {
          const double2 x2 = reinterpret_cast<const double2 *>(crow)[256 * e];
          cl[e] = x2.x;
          ch[e] = x2.y;
        }
      } else {
        ch[e] = crow[256 * e + H];
      }
#endif
    }
  };
  auto load_row_b = [&]() {
#pragma unroll
    for (int e = 0; e < 16; e++) {
#if RS_MAC3_ABLATE & 1
      if (PAIRED ? e >= 8 : true) cl[e] = 3.0 + e;
      if (PAIRED && e >= 8) ch[e] = 5.0 + t;
#else
      if (PAIRED) {
        if (e >= 8) {
          const double2 x2 = reinterpret_cast<const double2 *>(crow)[256 * e];
          cl[e] = x2.x;
          ch[e] = x2.y;
        }
      } else {
        cl[e] = crow[256 * e];
      }
#endif
    }
  };
  // Software pipeline over the terms of the chunk, one term deep: the spectrum of term t is parked in tile t % 2 and
  // multiplied into the accumulators during iteration t + 1, AFTER that iteration's plaintext-row loads have been
  // issued and BEFORE its transform, so the ciphertext loads of term t (issued before the transform of term t) have a
  // whole term to land and the row loads of term t + 1 fly during the multiply-accumulate.
  u64x2 ct[2][8];
  const bool temporal = a.ct_temporal != 0;
  auto issue_ct = [&]() {
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int i = 0; i < 8; i++) {
#if RS_MAC3_ABLATE & 2  // experiment: no ciphertext traffic (wrong results)
        ct[c][i] = u64x2{12345ull + i, 6789ull + c};
#else
        const u64x2 *cp = reinterpret_cast<const u64x2 *>(ctp + c * comp) + lane + 64 * i;
        ct[c][i] = temporal ? *cp : stream_load(cp);
#endif
      }
    ctp += enc_words;
  };
  int since = 0;
  auto mac = [&](const double *tile) {
    const int p0 = r0 + (r0 >> 4) + 2 * lane + (lane >> 3);  // px(r0 + 2 lane)
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const double u0 = tile[p0 + 136 * i], u1 = tile[p0 + 136 * i + 1];
#pragma unroll
      for (int c = 0; c < 2; c++) {
        acc[c][2 * i] += mulmod(from_u64(ct[c][i].x), u0, mod);
        acc[c][2 * i + 1] += mulmod(from_u64(ct[c][i].y), u1, mod);
      }
    }
    if (++since >= a.acc_period) {
      since = 0;
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[c][i] = reduce(acc[c][i], mod);
    }
  };
  constexpr int TILE = H + H / 16;
  for (unsigned long long tt = tbeg; tt < tend; tt++) {
    double *tile = s + (int)((tt - tbeg) & 1) * TILE;
    double v[16];
    if (LOGN == 13) {
      load_row_a();
      mem_fence();
      if (tt > tbeg) mac(s + (int)((tt - tbeg + 1) & 1) * TILE);  // term tt - 1
      mem_fence();
      load_row_b();
      crow += (size_t)L * n;
      mem_fence();
      // stage 0 (gap 4096): this half's operand of the 4096-point sub-transform, x[n'] + (+-w0) x[n' + 4096] (the sign of
      // the half rides on the twiddle: mulmod(a, -w) = -mulmod(a, w) exactly).  The reductions the mask asks for are whole
      // guarded passes over the registers: inside the element loops the compiler turns them into compute-and-select.
      if (red_mask & 1u) {
#pragma unroll
        for (int e = 0; e < 16; e++) ch[e] = reduce(ch[e], mod);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {
        ch[e] = mulmod(ch[e], w0s, mod);
        pin(ch[e]);
      }
      if (red_mask & 1u) {
#pragma unroll
        for (int e = 0; e < 16; e++) cl[e] = reduce(cl[e], mod);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {
        v[e] = cl[e] + ch[e];
        pin(v[e]);
      }
    } else {
      // stages 0 (gap 8192) and 1 (gap 4096) on x[n'], x[n' + 4096], x[n' + 8192], x[n' + 12288], n' = t + 256 e: the two
      // operands multiplied by stage 0's twiddle are requested before the previous term's multiply-accumulate, the
      // other two after it, one at a time (all 64 words at once do not fit beside the accumulators)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        cl[e] = crow[256 * e + 2 * H];
        ch[e] = crow[256 * e + 3 * H];
      }
      mem_fence();
      if (tt > tbeg) mac(s + (int)((tt - tbeg + 1) & 1) * TILE);  // term tt - 1
      mem_fence();
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = crow[256 * e];
      mem_fence();
      if (red_mask & 1u) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
          cl[e] = reduce(cl[e], mod);
          ch[e] = reduce(ch[e], mod);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {  // (+-w0) x2, (+-w0) x3: the sign of this quarter's half of stage 0 rides on the twiddle
        cl[e] = mulmod(cl[e], w0s, mod);
        ch[e] = mulmod(ch[e], w0s, mod);
        pin(cl[e]);
        pin(ch[e]);
      }
      if (red_mask & 1u) {
#pragma unroll
        for (int e = 0; e < 16; e++) v[e] = reduce(v[e], mod);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {  // u0 = x0 +- w0 x2
        cl[e] = v[e] + cl[e];
        pin(cl[e]);
      }
      mem_fence();
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = crow[256 * e + H];
      crow += (size_t)L * n;
      mem_fence();
      if (red_mask & 1u) {
#pragma unroll
        for (int e = 0; e < 16; e++) v[e] = reduce(v[e], mod);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {  // u1 = x1 +- w0 x3
        ch[e] = v[e] + ch[e];
        pin(ch[e]);
      }
      if (red_mask & 2u) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
          ch[e] = reduce(ch[e], mod);
          cl[e] = reduce(cl[e], mod);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; e++) {  // stage 1: v = u0 + (+-w1) u1
        v[e] = cl[e] + mulmod(ch[e], w1s, mod);
        pin(v[e]);
      }
    }
    mem_fence();
    issue_ct();  // after the row registers are dead: the two never overlap
    mem_fence();
#if RS_MAC3_ABLATE & 4  // experiment: no transform (wrong results)
    tile[17 * t] = v[0] + v[5] + v[9] + v[15];
    wave_sync();
    continue;
#endif
    // round 1: stages LOGP..LOGP+3 on elements t + 256 e (uniform twiddles)
    reg_fwd_stages<4, true>(v, mod, red_mask >> LOGP, [&](int k, int bk) { return tw1[(1 << k) - 1 + bk]; });
    {  // tile tt % 2 was last read by the multiply-accumulate of term tt - 2, two barriers ago
      const int pb = t + (t >> 4);
#pragma unroll
      for (int e = 0; e < 16; e++) tile[pb + 272 * e] = v[e];
    }
    __syncthreads();
    {  // round 2: stages 5..8 on hi*256 + lo + 16 e
      const int pb = hi * 272 + lo;
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = tile[pb + 17 * e];
      reg_fwd_stages<4, true>(v, mod, red_mask >> (LOGP + 4), [&](int k, int bk) { return twl[(root << (4 + k)) + (hi << k) + bk]; });
#pragma unroll
      for (int e = 0; e < 16; e++) tile[pb + 17 * e] = v[e];
    }
    wave_sync();  // a round-2 group (256 elements) is 16 consecutive threads, who also own it in round 3: no workgroup barrier
    {  // round 3: stages 9..12 on 16 consecutive points, parked for the wave-private transposition
      const int pb = 17 * t;
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = tile[pb + e];
      reg_fwd_stages<4, true>(v, mod, red_mask >> (LOGP + 8), [&](int k, int bk) { return tw3[(1 << k) - 1 + bk]; });
      if (a.reduce_u) {  // a guarded pass: as a per-element choice it becomes compute-and-select
#pragma unroll
        for (int e = 0; e < 16; e++) v[e] = reduce(v[e], mod);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) tile[pb + e] = v[e];
    }
    wave_sync();
  }
  if (tend > tbeg) mac(s + (int)((tend - tbeg + 1) & 1) * TILE);  // the last term
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int i = 0; i < 8; i++) {
      u64x2 o;
      o.x = to_u64(canon(acc[c][2 * i], mod));
      o.y = to_u64(canon(acc[c][2 * i + 1], mod));
      reinterpret_cast<u64x2 *>(part + c * comp + r0)[lane + 64 * i] = o;
    }
