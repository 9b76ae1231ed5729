// The kernel of cf_conv3x3_f16.hip, included there twice: as conv3x3_f16x3_kernel(Conv3F) and, with CF_CONV3_GROUPED, as
// conv3x3_f16x3_kernel_grouped(Conv3F, Conv3G) - the same text, so the plain kernel's code does not change when the grouped
// form is touched, and the grouped form differs only in where a workgroup finds its tile index and its operands.
template <int WC, int WP, int WK, int RT, int NU, bool DB, int MINB, bool T2, int CT = 2, bool S2 = false, bool ROOT = false,
          bool PROJ = false>
#if CF_CONV3_GROUPED
__global__ __launch_bounds__(64 * WC * WP * WK, MINB) void conv3x3_f16x3_kernel_grouped(Conv3F p, const Conv3G g) {
  static_assert(!S2 && !ROOT && !PROJ, "grouped form: stride 1, no fused Root / projection");
#else
__global__ __launch_bounds__(64 * WC * WP * WK, MINB) void conv3x3_f16x3_kernel(Conv3F p) {
#endif
  static_assert(!ROOT || (WK == 1 && RT == 2 && !S2 && 64 * WC * WP * WK == 256), "Root fusion: 64-channel waves, 4 waves, every channel of a pixel in the workgroup");
  static_assert(!PROJ || (!S2 && !ROOT), "projection k-steps: stride 1, no fused Root");
  constexpr int NT = 64 * WC * WP * WK;     // 4 waves, or 8 (WP doubled: two pixel groups share each weight fragment through L1)
  static_assert(NT == 256 || NT == 512, "4 or 8 waves per workgroup");
  static_assert(!S2 || (T2 && WK == 1), "stride 2: tiled form, no K split");
  constexpr int R = 32 * CT * WP;
  constexpr int PW2 = S2 ? 33 : 18;         // T2: entries per patch row (16 + 2; stride 2: 17 odd + 16 even input columns)
  constexpr int PYS = S2 ? 2 : 1;           // patch rows per output row
  constexpr int ROWB = 64 * WK + 16;        // per patch row: WK x (16 hi + 16 lo f16) + pad (odd multiple of 16 B)
  constexpr int UPR = 4 * WK;               // 16-byte fp32 units per patch row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  // the wave index is wave-uniform: read through readfirstlane so that everything derived from it (the wave's channel
  // group, its weight tile addresses, its k-steps) is scalar - SGPRs and scalar ALU instead of per-lane registers
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int wk = wave % WK, wp = (wave / WK) % WP, wc = wave / (WK * WP);
  // consecutive tiles on ONE XCD (cf_xcd_remap): neighbouring patches overlap, and every round
  // re-touches the same rows - both should hit that XCD's L2
#if CF_CONV3_GROUPED
  // workgroup b = tile b % n_tiles of group b / n_tiles (uniform: scalar loads from the argument block); everything below is
  // group-local - only the operands and the first output row are the group's
  const int grp = blockIdx.x / g.n_tiles;
  p.x = g.x[grp];
  p.weight = g.weight[grp];
  p.bias = g.bias[grp];
  p.in_scale = g.in_scale[grp];
  p.out_scale = g.out_scale[grp];
  p.out += (size_t)grp * p.M * p.out_stride;
  const int bid = cf_xcd_remap(blockIdx.x - grp * g.n_tiles, g.n_tiles);
#else
  const int bid = cf_xcd_remap(blockIdx.x, gridDim.x);
#endif
  int m0 = bid * R;                         // flat: first pixel; T2: first pixel of the image + tile origin below
  int ty0 = 0, tx0 = 0;
  if (T2) {
    const int per_img = p.tiles_x * p.tiles_y;
    const int b = bid / per_img, rem = bid - b * per_img;
    ty0 = (rem / p.tiles_x) * (R / 16);
    tx0 = (rem % p.tiles_x) * 16;
    m0 = b * p.HW;
  }
  const int m0i = S2 ? (m0 / p.HW) * p.HWi : m0;   // first pixel of the image in the INPUT map
  const int rt0 = (blockIdx.y * WC + wc) * RT;
  const bool w_ok = rt0 < p.n_rt;
  const int bufb = (p.PR + 1) * ROWB;       // + the zero row
  const int zrow = p.PR * ROWB + wk * 64 + h * 16;

  // zero rows of both buffers
  if (tid < ROWB / 4) {
    *reinterpret_cast<unsigned*>(smem + p.PR * ROWB + tid * 4) = 0u;
    if (DB) *reinterpret_cast<unsigned*>(smem + bufb + p.PR * ROWB + tid * 4) = 0u;
  }

  // ---- staging role: NU (patch row, 4-channel unit) pairs per thread
  int goff[NU];                              // element offset of the unit in x for round 0, -1 = zeros
#pragma unroll
  for (int it = 0; it < NU; ++it) {
    const int u = tid + NT * it;
    const int row = u / UPR, q = u % UPR;
    if (S2) {
      const int e = row % PW2;
      const int y = 2 * ty0 - 1 + row / PW2, x = e < 17 ? 2 * (tx0 + e) - 1 : 2 * (tx0 + e - 17);
      const bool ok = row < p.PR && (unsigned)y < (unsigned)p.Hi && (unsigned)x < (unsigned)p.Wi;
      goff[it] = ok ? (m0i + y * p.Wi + x) * p.x_stride + 4 * q : -1;
    } else if (T2) {
      const int y = ty0 - 1 + row / PW2, x = tx0 - 1 + row % PW2;
      const bool ok = row < p.PR && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
      goff[it] = ok ? (m0 + y * p.W + x) * p.x_stride + 4 * q : -1;
    } else {
      const int g = m0 - p.W - 1 + row;
      goff[it] = (row < p.PR && g >= 0 && g < p.M) ? g * p.x_stride + 4 * q : -1;
    }
  }
  // the next round's patch is staged in two halves (loads of the first half fly over taps 0-3, those of
  // the second over taps 4-8), so only half of the raw registers are live at any time.  The loads are
  // UNCONDITIONAL - a unit outside the image reads a valid dummy address and is zeroed when it is split - so no
  // exec-masked memory instruction sits inside the scheduling-pinned loop ("glitch")
  constexpr int NH0 = (NU + 1) / 2;
  f32x4 raw[NU];
  auto load_patch = [&](int r, int lo, int hi) {
    const int c0 = r * 16 * WK;
#pragma unroll
    for (int it = 0; it < NU; ++it) {
      if (it < lo || it >= hi) continue;
      raw[it] = *reinterpret_cast<const f32x4*>(p.x + max(goff[it], 0) + c0);
    }
  };
  auto store_patch = [&](unsigned char* buf, int lo, int hi) {
    int tid_s = threadIdx.x;                 // (laundered: the NU destination addresses are re-derived per call - 3 ALU
    asm volatile("" : "+v"(tid_s));          //  instructions each - instead of living in registers / scratch all loop long)
#pragma unroll
    for (int it = 0; it < NU; ++it) {
      if (it < lo || it >= hi) continue;
      const int u = tid_s + NT * it;
      const int row = u / UPR, q = u % UPR;
      if (row < p.PR) {
        const f32x4 xs = goff[it] >= 0 ? raw[it] * p.in_scale : f32x4{0.f, 0.f, 0.f, 0.f};   // (a select: the dummy read may hold anything)
        uint2 hi2, lo2;
        split2(xs[0], xs[1], hi2.x, lo2.x);
        split2(xs[2], xs[3], hi2.y, lo2.y);
        unsigned char* o = buf + row * ROWB + (q >> 2) * 64 + (q & 3) * 8;
        *reinterpret_cast<uint2*>(o) = hi2;
        *reinterpret_cast<uint2*>(o + 32) = lo2;
      }
    }
  };

  // ---- MFMA role: per column tile the patch row of this lane's pixel and its 9-bit tap validity
  int rowb[CT];
  unsigned vmask[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int pl = wp * (32 * CT) + ct * 32 + li;
    const int m = m0 + pl;
    rowb[ct] = (T2 ? (pl >> 4) * (PYS * PW2) + (pl & 15) : pl) * ROWB + wk * 64 + h * 16;
    unsigned mk = 0;
    if (T2) {
      mk = 0x1ffu;                           // the frame is part of the patch
    } else if (m < p.M) {
      const int rem = m % p.HW;
      const int y = rem / p.W, x = rem - y * p.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if ((unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W) mk |= 1u << t;
      }
    }
    vmask[ct] = mk;
  }

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

  // weight fragments three taps ahead: set (t % 3) holds tap t
  f16x8 wh[3][RT], wl[3][RT];
  const int ks_last = (p.n_rounds * WK - WK + wk) * 9 + 8;      // this wave's last k-step
  // fragment address = scalar tile base (row tile, k-step: uniform) + 16 * lane + 1 KiB for the lo plane: one per-lane
  // 32-bit offset register serves every weight load of the kernel
  const unsigned lane16 = (unsigned)lane * 16u;
  auto load_w = [&](f16x8 (&dh)[RT], f16x8 (&dl)[RT], int ks) {
    ks = min(ks, ks_last);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const unsigned char* base = p.weight + ((size_t)(w_ok ? rt0 + rt : 0) * p.n_ks + ks) * 2048;
      dh[rt] = *reinterpret_cast<const f16x8*>(base + lane16);
      dl[rt] = *reinterpret_cast<const f16x8*>(base + 1024 + lane16);
    }
  };

  load_patch(0, 0, NU);
#pragma unroll
  for (int t = 0; t < 3; ++t) load_w(wh[t], wl[t], wk * 9 + t);
  store_patch(smem, 0, NU);
  __syncthreads();

  for (int r = 0; r < p.n_rounds; ++r) {
    const unsigned char* cur = smem + (DB ? (r & 1) * bufb : 0);
    unsigned char* nxt = smem + (DB ? ((r + 1) & 1) * bufb : 0);
    const bool more = r + 1 < p.n_rounds;
    if (more) load_patch(r + 1, 0, NH0);
    const int ks0 = (r * WK + wk) * 9;
    // B fragments: the hi plane one tap ahead (xh[t & 1]), the lo plane - needed only by the third
    // sweep - at the start of its tap; weights three taps ahead.  The sched_barrier after every tap
    // keeps the compiler from sinking those prefetches back down to their first use
    f16x8 xh[2][CT], xl[CT];
    auto x_addr = [&](int ct, int t, int toff) { return (T2 || ((vmask[ct] >> t) & 1u)) ? rowb[ct] + toff : zrow; };
    // stride 2: entry {px, 17 + px, px + 1} of patch row 2 py + dy (compile-time per tap)
    auto s2_off = [](int t) { return ((t / 3) * PW2 + (t % 3 == 0 ? 0 : t % 3 == 1 ? 17 : 1)) * ROWB; };
    int toff = 0;                            // ((t / 3) * W + t % 3) * ROWB, built incrementally
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) xh[0][ct] = *reinterpret_cast<const f16x8*>(cur + x_addr(ct, 0, 0));
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) xl[ct] = *reinterpret_cast<const f16x8*>(cur + x_addr(ct, t, toff) + 32);
      if (S2) toff = s2_off(t + 1);
      else toff += (t % 3 == 2) ? ((T2 ? PW2 : p.W) - 2) * ROWB : ROWB;
      if (t + 1 < 9) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          xh[(t + 1) & 1][ct] = *reinterpret_cast<const f16x8*>(cur + x_addr(ct, t + 1, toff));
      }
      // three independent sweeps over the tiles: no MFMA waits on the one issued just before it
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          accs[rt][ct] = CF_MFMA_F16(wl[t % 3][rt], xh[t & 1][ct], accs[rt][ct]);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          accm[rt][ct] = CF_MFMA_F16(wh[t % 3][rt], xh[t & 1][ct], accm[rt][ct]);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          accs[rt][ct] = CF_MFMA_F16(wh[t % 3][rt], xl[ct], accs[rt][ct]);
      // tap t+3 of this round, or tap t-6 of the next one (same set either way)
      load_w(wh[t % 3], wl[t % 3], t + 3 < 9 ? ks0 + t + 3 : ks0 + 9 * WK + t - 6);
      if (DB && t == 3 && more) {            // first half of the next patch: split + store, then request the rest
        store_patch(nxt, 0, NH0);
        load_patch(r + 1, NH0, NU);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!DB) {
      __syncthreads();                       // single buffer: everyone is done reading it
      if (more) {
        store_patch(nxt, 0, NH0);
        load_patch(r + 1, NH0, NU);
      }
    }
    if (more) store_patch(nxt, NH0, NU);
    __syncthreads();
  }

  // ---- PROJ: the projection's k-steps, behind the 3x3 part (the patch is dead: its memory holds the B tiles)
  if constexpr (PROJ) {
    constexpr int BROW = 144;                // B tile: 64 f16 + 16 B per pixel row and plane
    constexpr int BPLANE = 32 * BROW;
    constexpr int REG = 2 * BPLANE;          // hi and lo plane of one piece: 9216 B
    constexpr int NG = WC * WK;              // waves of a pixel group
    int tid_p = threadIdx.x;                 // (every lane-derived index re-derived here, as in the epilogues: nothing of
    asm volatile("" : "+v"(tid_p));          //  this phase lives in registers across the main loop)
    const int lane = tid_p & 63, li = lane & 31, h = lane >> 5;
    const int gw = wc * WK + wk;
    unsigned char* myreg = smem + (gw * WP + wp) * REG;
    const int chunk = lane & 15, psub = lane >> 4;       // 16 lanes = one pixel's 64 channels, 4 pixels per instruction
    const int n_pieces = (p.proj_nks + 3) >> 2;           // (the last piece may hold 32 channels: level 2)
    auto group_sync = [&]() {
      if (NG > 1) __syncthreads();
      else cf_wave_lds_sync();
    };
    f16x8 pwh[4][RT], pwl[4][RT];
    auto load_pw = [&](int piece) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ks = p.proj_ks0 + min(piece * 4 + kk, p.proj_nks - 1);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const unsigned char* base = p.weight + ((long)(w_ok ? rt0 + rt : 0) * p.n_ks + ks) * 2048;
          pwh[kk][rt] = *reinterpret_cast<const f16x8*>(base + (unsigned)lane * 16u);
          pwl[kk][rt] = *reinterpret_cast<const f16x8*>(base + 1024 + (unsigned)lane * 16u);
        }
      }
    };
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      for (int e0 = 0; e0 < n_pieces; e0 += NG) {
        group_sync();                        // the previous round's fragments have been read: the regions are free
        const int e = e0 + gw;
        if (e < n_pieces) {
          const int cw = min(64, p.proj_ch - e * 64);
          // (two batches of four rows: eight rows in flight beside the accumulators and the weight fragments spill)
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            f32x4 xv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pl = wp * (32 * CT) + ct * 32 + (hb * 4 + j) * 4 + psub;
              int m = m0 + pl;
              bool ok = chunk * 4 < cw;
              if (T2) {
                const int y = ty0 + (pl >> 4), x = tx0 + (pl & 15);
                ok = ok && y < p.H && x < p.W;
                m = m0 + y * p.W + x;
              } else {
                ok = ok && m < p.M;
              }
              xv[j] = ok ? *reinterpret_cast<const f32x4*>(p.proj_x + (size_t)m * p.proj_c + e * 64 + chunk * 4)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const f32x4 xs = xv[j] * p.in_scale;
              uint2 hi2, lo2;
              split2(xs[0], xs[1], hi2.x, lo2.x);
              split2(xs[2], xs[3], hi2.y, lo2.y);
              unsigned char* o = myreg + ((hb * 4 + j) * 4 + psub) * BROW + chunk * 8;
              *reinterpret_cast<uint2*>(o) = hi2;
              *reinterpret_cast<uint2*>(o + BPLANE) = lo2;
            }
            asm volatile("" ::: "memory");   // (the next batch / the weight fragments are requested behind these stores)
          }
        }
        const int np = min(NG, n_pieces - e0);
        int i = wk;
        if (i < np) load_pw(e0 + i);         // (requested in front of the barrier)
        group_sync();
        for (; i < np; i += WK) {
          const unsigned char* reg = smem + (i * WP + wp) * REG + li * BROW + h * 16;
          const int nk = min(4, p.proj_nks - (e0 + i) * 4);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            if (kk < nk) {
              const f16x8 bh = *reinterpret_cast<const f16x8*>(reg + kk * 32);
              const f16x8 bl = *reinterpret_cast<const f16x8*>(reg + kk * 32 + BPLANE);
#pragma unroll
              for (int rt = 0; rt < RT; ++rt) {
                accs[rt][ct] = CF_MFMA_F16(pwl[kk][rt], bh, accs[rt][ct]);
                accm[rt][ct] = CF_MFMA_F16(pwh[kk][rt], bh, accm[rt][ct]);
                accs[rt][ct] = CF_MFMA_F16(pwh[kk][rt], bl, accs[rt][ct]);
              }
            }
          }
          if (i + WK < np) load_pw(e0 + i + WK);
        }
      }
    }
    __syncthreads();                         // every region has been read: the memory becomes the K-split / epilogue tiles
  }

  // ---- K-split waves: partial sums -> LDS, added by wave wk == 0 in fixed order
  if (WK > 1) {
    float* red = reinterpret_cast<float*>(smem);     // [wave][rt][ct][16][64]
    if (wk > 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            red[(((wave * RT + rt) * CT + ct) * 16 + r) * 64 + lane] = accm[rt][ct][r] + accs[rt][ct][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s = accm[rt][ct][r] + accs[rt][ct][r];
#pragma unroll
          for (int k = 1; k < WK; ++k) s += red[((((wave + k) * RT + rt) * CT + ct) * 16 + r) * 64 + lane];
          accm[rt][ct][r] = s;
          accs[rt][ct][r] = 0.0f;
        }
  }

  // ---- epilogue, coalesced form: the accumulators hold 4 consecutive channels of 32 DIFFERENT pixels per register
  // group, so storing them directly writes 32-byte pieces 64 channels apart (and reads the residual the same way) -
  // measured 8-26 % of a workgroup's time in this phase.  Each wave transposes its 32 pixels x 32*RT channels through
  // a private LDS tile instead (LDS executes a wave's instructions in order: no barrier) and then writes / reads whole
  // pixel rows: 8*RT lanes cover one contiguous run of RT*128 bytes.
  if constexpr (ROOT) {
    constexpr int EROW = RT * 128 + 16;      // transposition tile: 64 channels x 4 B + 16 per pixel row
    constexpr int BROW = 144;                // B tile: 64 f16 + 16 B per pixel row and plane
    constexpr int BPLANE = 32 * BROW;
    constexpr int REG = 2 * BPLANE;          // one region (>= 32 * EROW): 9216 B
    static_assert(REG >= 32 * EROW, "region holds a transposition tile");
    constexpr int LPP = RT * 8, PPI = 64 / LPP;
    asm volatile("; cf_epilogue_begin" ::: "memory");
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int lane = tid_e & 63, wave = __builtin_amdgcn_readfirstlane(tid_e >> 6), li = lane & 31, h = lane >> 5;
    const int wp = wave % WP, wc = wave / WP;   // (WK == 1)
    unsigned char* r1 = smem + wave * 2 * REG;
    unsigned char* r2 = r1 + REG;
    const int chunk = lane % LPP, psub = lane / LPP;
    const int n = wc * 64 + chunk * 4;       // this lane's 4 channels: of x2 / x1 (phases 1-2) and of the Root's output (phase 4)
    const int nl = chunk * 4;                // ... inside the wave's 64
    const f32x4 bias4 = *reinterpret_cast<const f32x4*>(p.bias + n);
    const f32x4 rbias4 = *reinterpret_cast<const f32x4*>(p.root_bias + n);
    auto group_sync = [&]() {                // the WC waves of a pixel group exchange data (WC == 1: the wave alone)
      if (WC > 1) __syncthreads();
      else cf_wave_lds_sync();
    };
    auto pixel = [&](int ct, int ploc, int& m) {     // -> inside the map?
      const int pl = wp * (32 * CT) + ct * 32 + ploc;
      if (T2) {
        const int y = ty0 + (pl >> 4), x = tx0 + (pl & 15);
        m = m0 + y * p.W + x;
        return y < p.H && x < p.W;
      }
      m = m0 + pl;
      return m < p.M;
    };
    auto put_split = [&](unsigned char* reg, int ploc, const f32x4& v) {   // 4 channels of one pixel -> B tile (hi, lo)
      const f32x4 xs = v * p.root_in_scale;
      uint2 hi2, lo2;
      split2(xs[0], xs[1], hi2.x, lo2.x);
      split2(xs[2], xs[3], hi2.y, lo2.y);
      unsigned char* o = reg + ploc * BROW + nl * 2;
      *reinterpret_cast<uint2*>(o) = hi2;
      *reinterpret_cast<uint2*>(o + BPLANE) = lo2;
    };
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      group_sync();                          // (everybody is done with the previous column tile's regions)
      // the Root's first weight fragments are requested now: they arrive under phases 1-2
      f16x8 rwh[4][RT], rwl[4][RT];          // (set ks % 4; the loop is unrolled by 4, so the set index is static)
      auto load_rw = [&](f16x8 (&dh)[RT], f16x8 (&dl)[RT], int ks) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          dh[rt] = *wfrag16(p.root_w, wc * RT + rt, ks, 0, p.root_nks, lane);
          dl[rt] = *wfrag16(p.root_w, wc * RT + rt, ks, 1, p.root_nks, lane);
        }
      };
      load_rw(rwh[0], rwl[0], 0);
      load_rw(rwh[1], rwl[1], 1);
      // 1. this convolution's accumulators -> region 1, transposed
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (accm[rt][ct][g * 4 + e] + accs[rt][ct][g * 4 + e]) * p.out_scale;
          *reinterpret_cast<f32x4*>(r1 + li * EROW + (rt * 32 + 8 * g + 4 * h) * 4) = v;
        }
      cf_wave_lds_sync();
      // 2. whole pixel rows: x2 = ReLU(conv + bias + x1) -> region 2 as a B tile; x1 stays in registers.  All rows are
      //    read (and x1 requested) before the first is written, so no LDS read follows a write inside a phase
      f32x4 x1v[32 / PPI], x2v[32 / PPI];
#pragma unroll
      for (int it = 0; it < 32 / PPI; ++it) {
        const int ploc = it * PPI + psub;
        int m;
        const bool ok = pixel(ct, ploc, m);
        x2v[it] = *reinterpret_cast<const f32x4*>(r1 + ploc * EROW + chunk * 16);
        x1v[it] = ok ? *reinterpret_cast<const f32x4*>(p.residual + (size_t)m * p.res_stride + n) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      cf_wave_lds_sync();                    // region 1 has been read by every lane: it becomes x1's B tile below
#pragma unroll
      for (int it = 0; it < 32 / PPI; ++it) {
        const int ploc = it * PPI + psub;
        f32x4 v = x2v[it] + bias4 + x1v[it];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        if (p.out) {
          int m;
          if (pixel(ct, ploc, m)) *reinterpret_cast<f32x4*>(p.out + (size_t)m * p.out_stride + n) = v;
        }
        put_split(r2, ploc, v);
        put_split(r1, ploc, x1v[it]);
      }
      group_sync();
      // 3. the Root: 8 WC k-steps - x2 channels in order (the pieces of waves wc' = 0 .. WC-1 of this pixel group), then
      //    x1 channels - with the slot kernel's products in the slot kernel's order; this wave's 64 output channels
      f32x16 rm[RT], rs[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          rm[rt][r] = 0.0f;
          rs[rt][r] = 0.0f;
        }
#pragma unroll 4
      for (int ks = 0; ks < 8 * WC; ++ks) {
        const int piece = (ks >> 2) % WC, src = ks / (4 * WC);          // whose region, x2 (region 2) or x1 (region 1)
        const unsigned char* row = smem + ((piece * WP + wp) * 2 + (src == 0 ? 1 : 0)) * REG + li * BROW + (ks & 3) * 32 + h * 16;
        const f16x8 xh = *reinterpret_cast<const f16x8*>(row);
        const f16x8 xl = *reinterpret_cast<const f16x8*>(row + BPLANE);
        load_rw(rwh[(ks + 2) % 4], rwl[(ks + 2) % 4], min(ks + 2, p.root_nks - 1));   // weights two k-steps ahead
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          rs[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwl[ks % 4][rt], xh, rs[rt], 0, 0, 0);
          rs[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwh[ks % 4][rt], xl, rs[rt], 0, 0, 0);
          rm[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwh[ks % 4][rt], xh, rm[rt], 0, 0, 0);
        }
      }
      // 3b. the Tree's children (further sources of the Root): 64-channel pieces, WC at a time - wave wc fetches piece
      //     e0 + wc of these 32 pixels from HBM (whole rows, as the residual), splits it into its region 2, and after the
      //     barrier every wave multiplies the round's pieces in K order.  The weight fragments keep rotating through the four sets (a
      //     piece is 4 k-steps, so the set index stays static).
      {
        const int n_extra = (p.root_nks - 8 * WC) >> 2;      // 64-channel pieces of the children
        const int ch0 = p.root_xsrc_ch[0] >> 6;               // pieces of the first child
        int ksx = 8 * WC;
        for (int e0 = 0; e0 < n_extra; e0 += WC) {
          group_sync();                        // the previous k-steps' fragments have been read: regions are free
          const int e = e0 + wc;
          if (e < n_extra) {
            // (the rows are requested here, not a round ahead or in front of the barrier: eight more row registers live
            //  across either spill; the CU's other workgroup covers the latency)
            const bool first = e < ch0;
            const float* xs = first ? p.root_xsrc[0] : p.root_xsrc[1];
            const int xc = first ? p.root_xsrc_c[0] : p.root_xsrc_c[1];
            const int off = (first ? e : e - ch0) * 64 + nl;
            f32x4 xv[32 / PPI];
#pragma unroll
            for (int it = 0; it < 32 / PPI; ++it) {
              int m;
              const bool ok = pixel(ct, it * PPI + psub, m);
              xv[it] = ok ? *reinterpret_cast<const f32x4*>(xs + (size_t)m * xc + off) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int it = 0; it < 32 / PPI; ++it) put_split(r2, it * PPI + psub, xv[it]);
          }
          group_sync();
          const int np = min(WC, n_extra - e0);
          for (int i = 0; i < np; ++i) {
            const unsigned char* reg = smem + ((i * WP + wp) * 2 + 1) * REG + li * BROW + h * 16;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const f16x8 xh = *reinterpret_cast<const f16x8*>(reg + kk * 32);
              const f16x8 xl = *reinterpret_cast<const f16x8*>(reg + kk * 32 + BPLANE);
              load_rw(rwh[(kk + 2) % 4], rwl[(kk + 2) % 4], min(ksx + kk + 2, p.root_nks - 1));
#pragma unroll
              for (int rt = 0; rt < RT; ++rt) {
                rs[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwl[kk][rt], xh, rs[rt], 0, 0, 0);
                rs[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwh[kk][rt], xl, rs[rt], 0, 0, 0);
                rm[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(rwh[kk][rt], xh, rm[rt], 0, 0, 0);
              }
            }
            ksx += 4;
          }
        }
      }
      group_sync();                          // every B fragment has been read: region 2 becomes the output's transposition tile
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (rm[rt][g * 4 + e] + rs[rt][g * 4 + e]) * p.root_scale;
          *reinterpret_cast<f32x4*>(r2 + li * EROW + (rt * 32 + 8 * g + 4 * h) * 4) = v;
        }
      cf_wave_lds_sync();
#pragma unroll
      for (int it = 0; it < 32 / PPI; ++it) {
        const int ploc = it * PPI + psub;
        int m;
        const bool ok = pixel(ct, ploc, m);
        f32x4 v = *reinterpret_cast<const f32x4*>(r2 + ploc * EROW + chunk * 16) + rbias4;
        if (p.root_act == CF_ACT_RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        }
        if (ok) *reinterpret_cast<f32x4*>(p.root_out + (size_t)m * p.root_out_stride + n) = v;
      }
    }
    return;
  }

  constexpr bool coalesced = WK == 1 && NT == 256;   // (8-wave configuration: measured no better; K-split waves: direct)
  if (coalesced && w_ok) {
    constexpr int EROW = RT * 128 + 16;      // bytes per pixel row of the tile: +16 B so that 16 lanes hit 64 banks
    constexpr int LPP = RT * 8;              // lanes (16-byte chunks) per pixel
    constexpr int PPI = 64 / LPP;            // pixels per instruction
    asm volatile("; cf_epilogue_begin" ::: "memory");   // marker for tools/check_isa.py (no instruction)
    // every lane-derived index of the epilogue is RE-derived here from a laundered thread id: computed once at the top of
    // the kernel they would stay live (or be spilled to scratch) across the whole MFMA loop that never uses them
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int lane = tid_e & 63, wave = __builtin_amdgcn_readfirstlane(tid_e >> 6), li = lane & 31, h = lane >> 5;
    const int wp = (wave / WK) % WP, wc = wave / (WK * WP);
    const int rt0 = (blockIdx.y * WC + wc) * RT;
    unsigned char* eb = smem + wave * 32 * EROW;
    const int chunk = lane % LPP, psub = lane / LPP;
    const int n = rt0 * 32 + chunk * 4;
    const bool n_ok = n < p.N;
    f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.N) bias4[e] = p.bias[n + e];
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
        const int pl = wp * (32 * CT) + ct * 32 + ploc;
        int m = m0 + pl;
        bool ok = n_ok;
        if (T2) {
          const int y = ty0 + (pl >> 4), x = tx0 + (pl & 15);
          ok = ok && y < p.H && x < p.W;
          m = m0 + y * p.W + x;
        } else {
          ok = ok && m < p.M;
        }
        f32x4 v = *reinterpret_cast<const f32x4*>(eb + ploc * EROW + chunk * 16) + bias4;
        if (ok && n + 3 < p.N) {
          if (p.residual) v += *reinterpret_cast<const f32x4*>(p.residual + (size_t)m * p.res_stride + n);
          if (p.act == CF_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
          }
          *reinterpret_cast<f32x4*>(p.out + (size_t)m * p.out_stride + n) = v;
        } else if (ok) {                     // last, partial group of channels (N = 27): element by element
          for (int e = 0; e < 4 && n + e < p.N; ++e) {
            float x = v[e];
            if (p.residual) x += p.residual[(size_t)m * p.res_stride + n + e];
            if (p.act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
            p.out[(size_t)m * p.out_stride + n + e] = x;
          }
        }
      }
    }
  }

  // ---- epilogue, direct form (K-split waves, N not a multiple of 4): lane = pixel, register group g = 4 consecutive channels
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    if (coalesced) break;
    const int pl = wp * (32 * CT) + ct * 32 + li;
    int m = m0 + pl;
    if (T2) {
      const int y = ty0 + (pl >> 4), x = tx0 + (pl & 15);
      if (y >= p.H || x >= p.W) continue;
      m = m0 + y * p.W + x;
    } else if (m >= p.M) {
      continue;
    }
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
          if (p.residual) v += *reinterpret_cast<const f32x4*>(p.residual + (size_t)m * p.res_stride + n);
          if (p.act == CF_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
          }
          *reinterpret_cast<f32x4*>(p.out + (size_t)m * p.out_stride + n) = v;
        } else {
          for (int e = 0; e < 4 && n + e < p.N; ++e) {
            float x = v[e] + p.bias[n + e];
            if (p.residual) x += p.residual[(size_t)m * p.res_stride + n + e];
            if (p.act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
            p.out[(size_t)m * p.out_stride + n + e] = x;
          }
        }
      }
  }
}

