// The DCN kernel of cf_gemm_f16.hip, included there twice: as dcn_f16x3_kernel(DcnF) and, with CF_DCN_GROUPED, as
// dcn_f16x3_kernel_grouped(DcnF, DcnG) - the same text, so the plain kernel's code does not change when the grouped form is
// touched; the grouped form differs only in where a workgroup finds its tile index, its operands and its rows.
template <int WC, int WP, int RT, bool COAL, int CT = 2>
#if CF_DCN_GROUPED
__global__ __launch_bounds__(256, 2) void dcn_f16x3_kernel_grouped(DcnF p, const DcnG g) {
#else
__global__ __launch_bounds__(256, 2) void dcn_f16x3_kernel(DcnF p) {
#endif
  static_assert(WC * WP == 4, "4 waves per workgroup");
  static_assert(CT == 2 || (CT == 1 && WP == 2), "half-size tiles: two pixel groups of 32");
  constexpr int PXB = 32 * CT * WP;
  constexpr int NP = PXB * 4 / 256;          // (pixel, 8-channel unit) pairs per thread and chunk
  constexpr int PLANE = PXB * FROWB;
  constexpr int BUF = 2 * PLANE;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF + PXB * 9 * 32];
  // sampling descriptor of one (pixel, tap), built ONCE per tile:
  //   dA = {element offset of the top-left corner (clamped into the image), step to the right corner
  //         (0 or C), step to the bottom corner (0 or W*C), 16 * sigmoid(mask)}
  //   dB = the four bilinear weights, ZERO where the corner lies outside the image
  // so the per-chunk staging is 8 unconditional loads (every address valid), 4 multiply-adds per
  // channel and the split - no floor / compare / branch in the K loop.
  f32x4* desc = reinterpret_cast<f32x4*>(smem + 2 * BUF);

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: scalar tile / weight addressing)
  const int li = lane & 31, h = lane >> 5;
  const int wc = wave / WP, wp = wave % WP;
  // consecutive pixel tiles on ONE XCD: the gathered rows of a tile and of its neighbours then meet
  // in that XCD's L2 instead of being fetched by all eight (hardware deals workgroups round-robin)
#if CF_DCN_GROUPED
  // workgroup b = tile b % n_tiles of group b / n_tiles (uniform: scalar loads from the argument block); m0 and every test
  // against M below are group-local - the group picks the operands and rows [g M, (g + 1) M) of om / out / partial
  const int grp = blockIdx.x / g.n_tiles;
  p.x = g.x[grp];
  p.weight = g.weight[grp];
  p.bias = g.bias[grp];
  p.in_scale = g.in_scale[grp];
  p.out_scale = g.out_scale[grp];
  p.om += (size_t)grp * p.M * p.om_stride;
  p.out += (size_t)grp * p.M * p.out_stride;
  if (p.partial) p.partial += (size_t)grp * p.M * (p.n_rt * 32);
  const int part_rows = g.M_all;              // rows of one z plane of partial
  const int m0 = cf_xcd_remap(blockIdx.x - grp * g.n_tiles, g.n_tiles) * PXB;
#else
  const int m0 = cf_xcd_remap(blockIdx.x, gridDim.x) * PXB;
#endif
  const int rt0 = (blockIdx.y * WC + wc) * RT;
  const bool w_ok = rt0 < p.n_rt;
  const int n_ks = p.n_chunks * 2;
  const int HW = p.H * p.W;

  // (all offset / mask values of the tile are requested before the first is used: one memory round trip for the phase
  //  instead of one per descriptor - it was 13 % of a 64-channel layer's workgroup time)
  constexpr int NDI = (PXB * 9 + 255) / 256;
  float omy[NDI], omx[NDI], omm[NDI];
#pragma unroll
  for (int it = 0; it < NDI; ++it) {
    const int i = min(tid + 256 * it, PXB * 9 - 1);
    const int r = i / 9, tap = i - r * 9;
    const float* om = p.om + (size_t)min(m0 + r, p.M - 1) * p.om_stride;
    omy[it] = om[2 * tap];
    omx[it] = om[2 * tap + 1];
    omm[it] = om[18 + tap];
  }
#pragma unroll
  for (int it = 0; it < NDI; ++it) {
    const int i = tid + 256 * it;
    if (i >= PXB * 9) break;
    const int r = i / 9, tap = i - r * 9;
    const int m = m0 + r;
    f32x4 dA = {0.0f, 0.0f, 0.0f, 0.0f}, dB = {0.0f, 0.0f, 0.0f, 0.0f};
    if (m < p.M) {
      const int b = m / HW, rem = m - b * HW;
      const int ho = rem / p.W, wo = rem - ho * p.W;
      const int ti = tap / 3, tj = tap - ti * 3;
      const float hf = (float)(ho - 1 + ti) + omy[it];
      const float wf = (float)(wo - 1 + tj) + omx[it];
      const bool inside = hf > -1.0f && hf < (float)p.H && wf > -1.0f && wf < (float)p.W;
      const float hfl = floorf(hf), wfl = floorf(wf);
      const int hl = inside ? (int)hfl : 0, wl = inside ? (int)wfl : 0;
      const float lh = hf - hfl, lw = wf - wfl, hh = 1.0f - lh, hw = 1.0f - lw;
      const bool t_ok = inside && hl >= 0, b_ok = inside && hl + 1 <= p.H - 1;
      const bool l_ok = wl >= 0, r_ok = wl + 1 <= p.W - 1;
      const int y0 = max(hl, 0), x0 = max(wl, 0);
      const int y1 = min(hl + 1, p.H - 1), x1 = min(wl + 1, p.W - 1);     // (hl + 1 >= 0 whenever inside)
      dA[0] = __int_as_float(((b * p.H + y0) * p.W + x0) * p.C);
      dA[1] = __int_as_float((max(x1, x0) - x0) * p.C);
      dA[2] = __int_as_float((max(y1, y0) - y0) * p.W * p.C);
      dA[3] = (p.mask_activated ? omm[it] : cf_sigmoid(omm[it])) * p.in_scale;
      dB[0] = (t_ok && l_ok) ? hh * hw : 0.0f;
      dB[1] = (t_ok && r_ok) ? hh * lw : 0.0f;
      dB[2] = (b_ok && l_ok) ? lh * hw : 0.0f;
      dB[3] = (b_ok && r_ok) ? lh * lw : 0.0f;
      // a corner that is clamped away shares its address with a valid one, so its weight must be zero:
      // true by construction (x1 == x0 only if !l_ok or !r_ok; y1 == y0 only if !t_ok or !b_ok)
    }
    desc[2 * i] = dA;
    desc[2 * i + 1] = dB;
  }
  __syncthreads();

  // corner samples are requested TWO chunks ahead (sets c & 1): the texture path, which bounds the
  // 64-channel layers, then always has a full chunk of requests queued behind the one being blended
  // (DEEP only for the two-pixel-group configuration: with WP = 1 the second set costs an occupancy
  //  step or spills and measured slower)
  // (... and for the half-size tiles, CT = 1: one set keeps them at 114 registers = FOUR workgroups per CU, which beats the
  //  deeper queue at three: 8 x 64 -> 64 at 112 x 200 106-108 vs 115-116 us, step 7.53 vs 7.63 ms)
  constexpr bool DEEP = WP == 2 && CT == 2;
  constexpr int NSET = DEEP ? 2 : 1;
  f32x4 cvs[NSET][NP][4][2];   // 4 corners x 8 channels
  f32x4 cws[NSET][NP];         // corner weights
  float cmks[NSET][NP];        // 16 * sigmoid(mask)
  auto load_b_pair = [&](int c, int i, f32x4 (&cv)[NP][4][2], f32x4 (&cw)[NP], float (&cmk)[NP]) __attribute__((always_inline)) {
    const int tap = c / p.chunks_per_tap;
    const int c0 = (c - tap * p.chunks_per_tap) * 32 + (tid & 3) * 8;
    {
      const int e = (((tid + 256 * i) >> 2) * 9 + tap) * 2;
      const f32x4 dA = desc[e];
      cw[i] = desc[e + 1];
      cmk[i] = dA[3];
      const float* a0 = p.x + (__float_as_int(dA[0]) + c0);
      const float* a1 = a0 + __float_as_int(dA[1]);
      const float* a2 = a0 + __float_as_int(dA[2]);
      const float* a3 = a2 + __float_as_int(dA[1]);
      cv[i][0][0] = *reinterpret_cast<const f32x4*>(a0);
      cv[i][0][1] = *reinterpret_cast<const f32x4*>(a0 + 4);
      cv[i][1][0] = *reinterpret_cast<const f32x4*>(a1);
      cv[i][1][1] = *reinterpret_cast<const f32x4*>(a1 + 4);
      cv[i][2][0] = *reinterpret_cast<const f32x4*>(a2);
      cv[i][2][1] = *reinterpret_cast<const f32x4*>(a2 + 4);
      cv[i][3][0] = *reinterpret_cast<const f32x4*>(a3);
      cv[i][3][1] = *reinterpret_cast<const f32x4*>(a3 + 4);
    }
  };
  auto load_b = [&](int c, f32x4 (&cv)[NP][4][2], f32x4 (&cw)[NP], float (&cmk)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) load_b_pair(c, i, cv, cw, cmk);
  };
  auto store_b = [&](unsigned char* buf, const f32x4 (&cv)[NP][4][2], const f32x4 (&cw)[NP], const float (&cmk)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int pr = tid + 256 * i;
      const float mk = cmk[i];   // the mask (x 2^4 activation scale) is applied after the 4-corner sum, as the reference does
      // explicit vector FMAs (v_pk_fma_f32: two channels per instruction)
      f32x4 v0 = cw[i][0] * cv[i][0][0], v1 = cw[i][0] * cv[i][0][1];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const f32x4 wk = {cw[i][k], cw[i][k], cw[i][k], cw[i][k]};
        v0 = __builtin_elementwise_fma(wk, cv[i][k][0], v0);
        v1 = __builtin_elementwise_fma(wk, cv[i][k][1], v1);
      }
      v0 *= mk;
      v1 *= mk;
      u32x4 hi, lo;                 // (the activation scale is already in mk)
      { unsigned th, tl; split2(v0[0], v0[1], th, tl); hi[0] = th; lo[0] = tl; }
      { unsigned th, tl; split2(v0[2], v0[3], th, tl); hi[1] = th; lo[1] = tl; }
      { unsigned th, tl; split2(v1[0], v1[1], th, tl); hi[2] = th; lo[2] = tl; }
      { unsigned th, tl; split2(v1[2], v1[3], th, tl); hi[3] = th; lo[3] = tl; }
      unsigned char* o = buf + (pr >> 2) * FROWB + (pr & 3) * 16;
      *reinterpret_cast<u32x4*>(o) = hi;
      *reinterpret_cast<u32x4*>(o + PLANE) = lo;
    }
  };

  f32x16 accm[RT][CT], accs[RT][CT];
#pragma unroll
  for (int a = 0; a < RT; ++a)
#pragma unroll
    for (int b = 0; b < CT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accm[a][b][r] = 0.0f;
        accs[a][b][r] = 0.0f;
      }
  f16x8 wh[2][RT], wl[2][RT];
  auto load_w = [&](f16x8 (&dh)[RT], f16x8 (&dl)[RT], int ks) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      dh[rt] = *wfrag16(p.weight, w_ok ? rt0 + rt : 0, ks, 0, n_ks, lane);
      dl[rt] = *wfrag16(p.weight, w_ok ? rt0 + rt : 0, ks, 1, n_ks, lane);
    }
  };
  auto mma_kstep = [&](const unsigned char* buf, int s, const f16x8 (&ah)[RT], const f16x8 (&al)[RT]) {
    f16x8 xh[CT], xl[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const unsigned char* row = buf + (wp * 32 * CT + ct * 32 + li) * FROWB + s * 32 + h * 16;
      xh[ct] = *reinterpret_cast<const f16x8*>(row);
      xl[ct] = *reinterpret_cast<const f16x8*>(row + PLANE);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[rt], xh[ct], accs[rt][ct], 0, 0, 0);
        accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xl[ct], accs[rt][ct], 0, 0, 0);
        accm[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xh[ct], accm[rt][ct], 0, 0, 0);
      }
  };

  // K split over gridDim.z (small maps with long K: 88 tiles x 144 chunks at 14x25 cannot fill the chip,
  // and one tile's chunk chain is latency-bound): this workgroup owns chunks [c_lo, c_hi)
  const int c_lo = (int)((long)p.n_chunks * blockIdx.z / gridDim.z);
  const int c_hi = (int)((long)p.n_chunks * (blockIdx.z + 1) / gridDim.z);
  // chunk j (relative to c_lo) lives in LDS buffer j & 1 and (DEEP) in register set j & 1
  const int n_own = c_hi - c_lo;
  load_b(c_lo, cvs[0], cws[0], cmks[0]);
  load_w(wh[0], wl[0], 2 * c_lo);
  load_w(wh[1], wl[1], 2 * c_lo + 1);
  if (DEEP && n_own > 1) load_b(c_lo + 1, cvs[NSET - 1], cws[NSET - 1], cmks[NSET - 1]);
  store_b(smem, cvs[0], cws[0], cmks[0]);
  if (n_own > NSET) load_b(c_lo + NSET, cvs[0], cws[0], cmks[0]);
  __syncthreads();
  // (an earlier form with exec-masked corner loads inside a pinned loop glitched when launched behind unrelated kernels,
  //  tools/stress_dcn.py: the loads below are unconditional)
  auto iteration = [&](int j, f32x4 (&cv)[NP][4][2], f32x4 (&cw)[NP], float (&cmk)[NP]) {
    // MFMAs of chunk j; then chunk j+1 (held in set cv) is blended into the other buffer and the set is
    // re-requested for chunk j+1+NSET
    unsigned char* cur = smem + (j & 1) * BUF;
    unsigned char* nxt = smem + ((j + 1) & 1) * BUF;
    const int c = c_lo + j;
    // Straight-line, hand-interleaved form for the single-pixel-group tiles (WP == 1: the 128- / 256-channel layers on the
    // 28 x 50 and 14 x 25 maps): every MFMA is followed by one PIECE of the next chunk's staging (blend of 8 channels x 4
    // corners, operand split + LDS store, the corner requests of the chunk after that) and a sched_barrier keeps it
    // there, so the MFMA executes while the wave issues the piece; indices are clamped instead of branching and every
    // load is unconditional (no exec-masked operand load inside a pinned loop).  Bit-identical to
    // the plain form.  Measured (tools/bench_dcn.py, same box): 256 -> 128 at 28 x 50: 86.4 vs 93.0 us; the two-group tiles
    // of the 64-channel layers LOSE with it (254 vs 212 us, 149 vs 131 us: every wait for a corner or an LDS fragment then
    // also holds back the wave's next MFMA), so they keep the compiler's order.
    if constexpr (WP == 1 && CT == 2)
    {
      f32x4 bv[2];                           // blended 8 channels of the pair in progress
      u32x4 bhi, blo;
      auto work = [&](int slot) __attribute__((always_inline)) {
        constexpr int NSTG = 4 * WP;         // staging pieces: 4 per (pixel, unit) pair
        if (slot < NSTG) {
          const int i = slot >> 2, part = slot & 3;
          if (part < 2) {                    // blend: 4 channels... x2 (one f32x4 half of the 8-channel unit), then the mask
            f32x4 v = cw[i][0] * cv[i][0][part];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
              const f32x4 wk4 = {cw[i][k], cw[i][k], cw[i][k], cw[i][k]};
              v = __builtin_elementwise_fma(wk4, cv[i][k][part], v);
            }
            bv[part] = v * cmk[i];
          } else {                           // split to fp16 hi / lo; the second half also stores the unit
            const int hf = part - 2;
            { unsigned th, tl; split2(bv[hf][0], bv[hf][1], th, tl); bhi[2 * hf] = th; blo[2 * hf] = tl; }
            { unsigned th, tl; split2(bv[hf][2], bv[hf][3], th, tl); bhi[2 * hf + 1] = th; blo[2 * hf + 1] = tl; }
            if (hf == 1) {
              const int pr = tid + 256 * i;
              unsigned char* o = nxt + (pr >> 2) * FROWB + (pr & 3) * 16;
              *reinterpret_cast<u32x4*>(o) = bhi;
              *reinterpret_cast<u32x4*>(o + PLANE) = blo;
            }
          }
        } else if (slot < NSTG + WP) {       // corner requests of chunk c + 1 + NSET into the set just consumed
          load_b_pair(min(c + 1 + NSET, c_hi - 1), slot - NSTG, cv, cw, cmk);
        }
      };
      auto kstep = [&](int s, const f16x8 (&ah)[RT], const f16x8 (&al)[RT]) __attribute__((always_inline)) {
        f16x8 xh[CT], xl[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const unsigned char* row = cur + (wp * 32 * CT + ct * 32 + li) * FROWB + s * 32 + h * 16;
          xh[ct] = *reinterpret_cast<const f16x8*>(row);
          xl[ct] = *reinterpret_cast<const f16x8*>(row + PLANE);
        }
        int slot = s * 6 * RT;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[rt], xh[ct], accs[rt][ct], 0, 0, 0);
            work(slot++);
            __builtin_amdgcn_sched_barrier(0);
            accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xl[ct], accs[rt][ct], 0, 0, 0);
            work(slot++);
            __builtin_amdgcn_sched_barrier(0);
            accm[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xh[ct], accm[rt][ct], 0, 0, 0);
            work(slot++);
            __builtin_amdgcn_sched_barrier(0);
          }
      };
      kstep(0, wh[0], wl[0]);
      load_w(wh[0], wl[0], min(2 * c + 2, 2 * c_hi - 2));
      __builtin_amdgcn_sched_barrier(0);
      kstep(1, wh[1], wl[1]);
      load_w(wh[1], wl[1], min(2 * c + 3, 2 * c_hi - 1));
      __syncthreads();
      return;
    }
    mma_kstep(cur, 0, wh[0], wl[0]);
    if (j + 1 < n_own) load_w(wh[0], wl[0], 2 * c + 2);
    mma_kstep(cur, 1, wh[1], wl[1]);
    if (j + 1 < n_own) {
      load_w(wh[1], wl[1], 2 * c + 3);
      store_b(nxt, cv, cw, cmk);
      if (j + 1 + NSET < n_own) load_b(c + 1 + NSET, cv, cw, cmk);
    }
    __syncthreads();
  };
  if (DEEP) {
    for (int j = 0; j < n_own; j += 2) {
      iteration(j, cvs[NSET - 1], cws[NSET - 1], cmks[NSET - 1]);     // chunk j+1 was requested into set 1
      if (j + 1 < n_own) iteration(j + 1, cvs[0], cws[0], cmks[0]);
    }
  } else {
    for (int j = 0; j < n_own; ++j) iteration(j, cvs[0], cws[0], cmks[0]);
  }

  if (gridDim.z > 1) {   // raw partial sums; scale / bias / activation happen in the reduction
    const int ns = p.n_rt * 32;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int m = m0 + wp * 32 * CT + ct * 32 + li;
      if (m >= p.M || !w_ok) continue;
#if CF_DCN_GROUPED
      float* o = p.partial + ((size_t)blockIdx.z * part_rows + m) * ns;
#else
      float* o = p.partial + ((size_t)blockIdx.z * p.M + m) * ns;
#endif
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = accm[rt][ct][g * 4 + e] + accs[rt][ct][g * 4 + e];
          *reinterpret_cast<f32x4*>(o + (rt0 + rt) * 32 + 8 * g + 4 * h) = v;
        }
    }
    return;
  }

  // Coalesced epilogue (as in cf_conv3x3_f16.hip): each wave transposes its 32 pixels x 32*RT channels through a private
  // LDS tile (free after the loop's last barrier) and writes whole pixel rows - RT*128 contiguous bytes per pixel
  // instead of 32-byte pieces - and the split-bf16 copy as 8-byte pieces that are contiguous across lanes.
  constexpr bool coalesced = COAL;        // (the host selects it: N % 4 == 0)
  if (coalesced && w_ok) {
    constexpr int EROW = RT * 128 + 16;
    constexpr int LPP = RT * 8, PPI = 64 / LPP;
    asm volatile("; cf_epilogue_begin" ::: "memory");   // marker for tools/check_isa.py (no instruction)
    unsigned char* eb = smem + wave * 32 * EROW;
    const int chunk = lane % LPP, psub = lane / LPP;
    const int n = rt0 * 32 + chunk * 4;
    const bool n_ok = n < p.N;
    f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n_ok) bias4 = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (ct) cf_wave_lds_sync();            // ... and every lane has read the previous tile before it is overwritten
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (accm[rt][ct][g * 4 + e] + accs[rt][ct][g * 4 + e]) * p.out_scale;
          *reinterpret_cast<f32x4*>(eb + li * EROW + (rt * 32 + 8 * g + 4 * h) * 4) = v;
        }
      cf_wave_lds_sync();                    // the tile is complete before any lane reads another lane's part ...
#pragma unroll
      for (int it = 0; it < 32 / PPI; ++it) {
        const int ploc = it * PPI + psub;
        const size_t m = (size_t)m0 + wp * 32 * CT + ct * 32 + ploc;
        f32x4 v = *reinterpret_cast<const f32x4*>(eb + ploc * EROW + chunk * 16) + bias4;
        if (n_ok && m < (size_t)p.M) {
          if (p.act == CF_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
          }
          *reinterpret_cast<f32x4*>(p.out + m * p.out_stride + n) = v;
          if (p.out_split) {   // hi = rne_bf16(v), lo = rne_bf16(v - hi): the head kernels' input format
            unsigned w[4];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const __bf16 h0 = (__bf16)v[2 * e], h1 = (__bf16)v[2 * e + 1];
              const __bf16 l0 = (__bf16)(v[2 * e] - (float)h0), l1 = (__bf16)(v[2 * e + 1] - (float)h1);
              w[e] = ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16) | __builtin_bit_cast(unsigned short, h0);
              w[2 + e] = ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16) | __builtin_bit_cast(unsigned short, l0);
            }
            unsigned* o = p.out_split + (m * 2 * p.split_stride + n) / 2;
            *reinterpret_cast<uint2*>(o) = uint2{w[0], w[1]};
            *reinterpret_cast<uint2*>(o + p.split_stride / 2) = uint2{w[2], w[3]};
          }
        }
      }
      if constexpr (RT == 1) {
        // the mx rows of the heads (cf_head_fused mx = 1) from the same tile: this wave holds one 32-channel block of its 32
        // pixels; lane l < 32 packs pixel l exactly as cf_pack_feat_mx would from `out` (same fp32 values: tile + bias, ReLU)
        if (p.out_mx && lane < 32) {
          const size_t m = (size_t)m0 + wp * 32 * CT + ct * 32 + lane;
          if (m < (size_t)p.M) {
            float v[32];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              f32x4 t = *reinterpret_cast<const f32x4*>(eb + lane * EROW + i * 16) + *reinterpret_cast<const f32x4*>(p.bias + rt0 * 32 + 4 * i);
#pragma unroll
              for (int e = 0; e < 4; ++e) v[4 * i + e] = p.act == CF_ACT_RELU ? fmaxf(t[e], 0.0f) : t[e];
            }
            mx_pack_block(v, p.out_mx + m * 272, rt0, p.mx_scale);
          }
        }
      }
    }
  }

#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int m = m0 + wp * 32 * CT + ct * 32 + li;
    if (coalesced) break;
    if (m >= p.M) continue;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = (rt0 + rt) * 32 + 8 * g + 4 * h;
        if (n >= p.N) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (accm[rt][ct][g * 4 + e] + accs[rt][ct][g * 4 + e]) * p.out_scale;
        if (n + 3 < p.N) {
          v += *reinterpret_cast<const f32x4*>(p.bias + n);
          if (p.act == CF_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
          }
          *reinterpret_cast<f32x4*>(p.out + (size_t)m * p.out_stride + n) = v;
          if (p.out_split) {   // hi = rne_bf16(v), lo = rne_bf16(v - hi): the head kernels' input format
            unsigned w[4];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const __bf16 h0 = (__bf16)v[2 * e], h1 = (__bf16)v[2 * e + 1];
              const __bf16 l0 = (__bf16)(v[2 * e] - (float)h0), l1 = (__bf16)(v[2 * e + 1] - (float)h1);
              w[e] = ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16) | __builtin_bit_cast(unsigned short, h0);
              w[2 + e] = ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16) | __builtin_bit_cast(unsigned short, l0);
            }
            unsigned* o = p.out_split + ((size_t)m * 2 * p.split_stride + n) / 2;
            *reinterpret_cast<uint2*>(o) = uint2{w[0], w[1]};
            *reinterpret_cast<uint2*>(o + p.split_stride / 2) = uint2{w[2], w[3]};
          }
        } else {
          for (int e = 0; e < 4 && n + e < p.N; ++e) {
            float x = v[e] + p.bias[n + e];
            if (p.act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
            p.out[(size_t)m * p.out_stride + n + e] = x;
          }
        }
      }
  }
}

