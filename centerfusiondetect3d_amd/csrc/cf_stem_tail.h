// cf_stem.hip, included INSIDE its kernels: level0 (P2) and level1 + max-pool (P3) over the base region a kernel has left in
// `base_lds`.  Shared as text rather than as a function so that the three-channel kernel's token stream - and with it its code
// object - is exactly what it was before the early-fusion kernel existed.  Expects in scope: p (StemK), base_lds, l0_lds, lane,
// wave, col, kg, b, oy0, ox0, y_l0, x_l0, interior.
  // ---- P2 weights / offsets: k-step = taps 2ks, 2ks+1; lane k group: tap 2ks + (kg >> 1), channels 8(kg & 1)..+8
  f16x8 w0h[5], w0l[5];
  int t0off[5];
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) {
    w0h[ks] = *sfrag(p.w_l0, ks * 2 + 0, lane);
    w0l[ks] = *sfrag(p.w_l0, ks * 2 + 1, lane);
    auto off = [](int tap) { tap = tap < 8 ? tap : 8; return ((tap / 3) * ST_RB + tap % 3) * ST_ROWB; };
    t0off[ks] = (kg & 2 ? off(2 * ks + 1) : off(2 * ks)) + (kg & 1) * 16;
  }
  const f32x4v bias_0 = *reinterpret_cast<const f32x4v*>(p.b_l0 + 4 * kg);
  __syncthreads();

  // ---- P2: level0 over the 17 x 17 region, two tiles in flight per wave
  constexpr int N0 = ST_R0 * ST_R0;                          // 289
  constexpr int NT0 = (N0 + 15) / 16;                        // 19
  for (int t0 = wave; t0 < NT0; t0 += 8) {
    int q[2], py[2], px[2];
    const unsigned char* src[2];
    f32x4v accm[2], accs[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      q[u] = min((t0 + 4 * u) * 16 + col, N0 - 1);
      py[u] = q[u] / ST_R0;
      px[u] = q[u] - py[u] * ST_R0;
      src[u] = base_lds + (py[u] * ST_RB + px[u]) * ST_ROWB;
      accm[u] = f32x4v{0.f, 0.f, 0.f, 0.f};
      accs[u] = accm[u];
    }
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      f16x8 xh[2], xl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        xh[u] = *reinterpret_cast<const f16x8*>(src[u] + t0off[ks]);
        xl[u] = *reinterpret_cast<const f16x8*>(src[u] + t0off[ks] + 32);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) accs[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0l[ks], xh[u], accs[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) accm[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0h[ks], xh[u], accm[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) accs[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0h[ks], xl[u], accs[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int y = y_l0 + py[u], x = x_l0 + px[u];
      const bool inside = interior || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W);
      f32x4v v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = inside ? fmaxf((accm[u][e] + accs[u][e]) * p.s_l0 + bias_0[e], 0.0f) : 0.0f;
      uint2 hi, lo;
      split4(v, hi, lo, p.a_l0);
      if ((t0 + 4 * u) * 16 + col < N0) {
        *reinterpret_cast<uint2*>(l0_lds + q[u] * ST_ROWB + 8 * kg) = hi;
        *reinterpret_cast<uint2*>(l0_lds + q[u] * ST_ROWB + 32 + 8 * kg) = lo;
      }
    }
  }

  // ---- P3 weights / offsets (stride 2: out (oy, ox) reads level0 region (2oy + ky, 2ox + kx)).
  //      Wave w owns the 16-channel half rt = w >> 1 of pixels 32 (w & 1) .. +32: one half's weights per wave
  const int rt = wave >> 1;
  f16x8 w1h[5], w1l[5];
  int t1off[5];
#pragma unroll
  for (int ks = 0; ks < 5; ++ks) {
    w1h[ks] = *sfrag(p.w_l1, (rt * 5 + ks) * 2 + 0, lane);
    w1l[ks] = *sfrag(p.w_l1, (rt * 5 + ks) * 2 + 1, lane);
    auto off = [](int tap) { tap = tap < 8 ? tap : 8; return ((tap / 3) * ST_R0 + tap % 3) * ST_ROWB; };
    t1off[ks] = (kg & 2 ? off(2 * ks + 1) : off(2 * ks)) + (kg & 1) * 16;
  }
  const f32x4v bias_1 = *reinterpret_cast<const f32x4v*>(p.b_l1 + 16 * rt + 4 * kg);
  __syncthreads();

  // ---- P3: level1, 64 output pixels x 32 channels
  {
    const unsigned char* src[2];
    f32x4v accm[2], accs[2];
    int oy[2], ox[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = (wave & 1) * 32 + u * 16 + col;
      oy[u] = q >> 3;
      ox[u] = q & 7;
      src[u] = l0_lds + ((2 * oy[u]) * ST_R0 + 2 * ox[u]) * ST_ROWB;
      accm[u] = f32x4v{0.f, 0.f, 0.f, 0.f};
      accs[u] = accm[u];
    }
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      f16x8 xh[2], xl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        xh[u] = *reinterpret_cast<const f16x8*>(src[u] + t1off[ks]);
        xl[u] = *reinterpret_cast<const f16x8*>(src[u] + t1off[ks] + 32);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) accs[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1l[ks], xh[u], accs[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) accm[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h[ks], xh[u], accm[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) accs[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h[ks], xl[u], accs[u], 0, 0, 0);
    }
    const int H1 = p.H / 2, W1 = p.W / 2;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int y = oy0 + oy[u], x = ox0 + ox[u];
      f32x4v v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf((accm[u][e] + accs[u][e]) * p.s_l1 + bias_1[e], 0.0f);
      if (y < H1 && x < W1) *reinterpret_cast<f32x4v*>(p.out + (((size_t)b * H1 + y) * W1 + x) * 32 + 16 * rt + 4 * kg) = v;
      // the level-2 Tree max-pools this map 2x2 (dla.py:96 downsample) - the only reader of that pool is its `project`: the
      // 16 pixels of the MFMA tile are two rows of 8, so a pool window is lanes {c, c + 1, c + 8, c + 9} of one k group:
      // two lane exchanges, and the even-column lanes of the upper row write the pooled pixel (floor semantics at odd sizes)
      if (p.out_pool) {
        f32x4v m = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m[e] = fmaxf(m[e], __shfl_xor(m[e], 1));
          m[e] = fmaxf(m[e], __shfl_xor(m[e], 8));
        }
        const int H2 = H1 / 2, W2 = W1 / 2, yp = y >> 1, xp = x >> 1;
        if ((col & 9) == 0 && yp < H2 && xp < W2)
          *reinterpret_cast<f32x4v*>(p.out_pool + (((size_t)b * H2 + yp) * W2 + xp) * 32 + 16 * rt + 4 * kg) = m;
      }
    }
  }
