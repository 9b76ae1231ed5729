// Training kernels of the DLA-34 stem (ops.stem_conv_bn_relu): the narrow convolutions of base.base_layer (7x7, 3 or 6 -> 16),
// base.level0 (3x3, 16 -> 16) and base.level1 (3x3 stride 2, 16 -> 32), padding (k - 1) / 2, no bias, exact fp32.
//
//   cf_stem_conv_forward      z (B,Ho,Wo,Cout) NHWC, the pre-BN map: one thread per output pixel, every output channel in registers,
//                             the weight in LDS as [tap][c][n] (a wave reads one address: a broadcast), v_fma_f32
//   cf_stem_conv_bwd_weight   gw (Cout,Cin,k,k): slab partials on v_mfma_f32_16x16x4_f32, added in slab order by a second launch
//   cf_stem_conv_bwd_data     gx (B,H,W,16) NHWC of the 3x3 layers: one thread per input pixel; under stride 2 a workgroup's pixels
//                             share the parity of their row and column and walk the taps of that parity alone
//
// k = 7 (stride 1, Cin <= 8): the input is the caller's NCHW image; with `radar` its last three channels are the (B,3,H/4,W/4)
// radar map sampled at (y >> 2, x >> 2) - F.interpolate(mode="nearest") of an exact 4x upsample - so the six-channel image is
// never written.  k = 3 (stride 1 or 2, Cin = 16): NHWC.  Cout = 16 or 32.  BatchNorm + ReLU are cf_bn_act_* (cf_base_bwd.hip).
// No float atomics in this file: every sum is taken in a fixed order, every result is bitwise reproducible.  Element offsets are
// 64-bit (one 16-channel map at batch 16, 448 x 800 is 92 M floats).
#include "cf_common.h"

namespace {

struct SGeo {
  int B, H, W, Cin, Cimg, Cout, Ho, Wo, k, stride, pad, Hr, Wr;   // Cimg: channels that come from x (the rest from the radar map)
};

int sgeo_check(const char* who, int B, int H, int W, int Cin, int Cout, int k, int stride, bool radar, SGeo* g) {
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  CF_REQUIRE((k == 7 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)),
             "%s: k=%d stride=%d (7x7 stride 1, or 3x3 stride 1 or 2)", who, k, stride);
  CF_REQUIRE(Cout == 16 || Cout == 32, "%s: Cout=%d must be 16 or 32", who, Cout);
  if (k == 7) {
    CF_REQUIRE(Cin > 0 && Cin <= 8, "%s: Cin=%d of a 7x7 layer must be 1..8", who, Cin);
    CF_REQUIRE(!radar || (Cin > 3 && H % 4 == 0 && W % 4 == 0), "%s: a radar map needs Cin > 3 and H, W multiples of 4", who);
  } else {
    CF_REQUIRE(Cin == 16, "%s: Cin=%d of a 3x3 layer must be 16", who, Cin);
    CF_REQUIRE(!radar, "%s: only the 7x7 layer reads a radar map", who);
  }
  g->B = B; g->H = H; g->W = W; g->Cin = Cin; g->Cout = Cout; g->k = k; g->stride = stride;
  g->Cimg = radar ? Cin - 3 : Cin;
  g->pad = (k - 1) / 2;
  g->Ho = (H + 2 * g->pad - k) / stride + 1;
  g->Wo = (W + 2 * g->pad - k) / stride + 1;
  g->Hr = H / 4; g->Wr = W / 4;
  CF_REQUIRE((long)B * H * W < (1L << 31), "%s: tensor too large (pixel counts are 32-bit, element offsets 64-bit)", who);
  return CF_OK;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int ST_COLS = 64, ST_ROWS = 4;   // pixels of a workgroup of the forward / data kernels: 64 columns of 4 rows, one row per wave

// ---------------------------------------------------------------------------------------------------------------------------
// forward
struct SfArgs {
  const float* x;
  const float* radar;
  const float* weight;   // raw (Cout, Cin, k, k)
  float* z;
  SGeo g;
};

template <int COUT, bool NHWC>
__global__ __launch_bounds__(256) void stem_conv_fwd_kernel(const SfArgs p) {
  extern __shared__ float wl[];                    // [tap][c][n]
  const SGeo& g = p.g;
  const int tid = threadIdx.x, kk = g.k * g.k;
  for (int i = tid; i < kk * g.Cin * COUT; i += 256) {
    const int n = i % COUT, rest = i / COUT, c = rest % g.Cin, tap = rest / g.Cin;
    wl[i] = p.weight[((size_t)n * g.Cin + c) * kk + tap];
  }
  __syncthreads();
  const int xo = blockIdx.y * ST_COLS + (tid & 63);
  const long row = (long)blockIdx.x * ST_ROWS + (tid >> 6);     // over B * Ho
  if (xo >= g.Wo || row >= (long)g.B * g.Ho) return;
  const int b = (int)(row / g.Ho), yo = (int)(row - (long)b * g.Ho);
  float acc[COUT];
#pragma unroll
  for (int n = 0; n < COUT; ++n) acc[n] = 0.0f;
  for (int ti = 0; ti < g.k; ++ti) {
    const int yy = yo * g.stride - g.pad + ti;
    if (yy < 0 || yy >= g.H) continue;
    for (int tj = 0; tj < g.k; ++tj) {
      const int xx = xo * g.stride - g.pad + tj;
      if (xx < 0 || xx >= g.W) continue;
      const float* wt = wl + (ti * g.k + tj) * g.Cin * COUT;
      if (NHWC) {
        const f32x4* xp = reinterpret_cast<const f32x4*>(p.x + (((size_t)b * g.H + yy) * g.W + xx) * g.Cin);
        for (int c4 = 0; c4 < g.Cin / 4; ++c4) {
          const f32x4 v = xp[c4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < COUT; ++n) acc[n] = fmaf(v[e], wt[(c4 * 4 + e) * COUT + n], acc[n]);
        }
      } else {
        for (int c = 0; c < g.Cin; ++c) {
          const float v = c < g.Cimg ? p.x[(((size_t)b * g.Cimg + c) * g.H + yy) * g.W + xx]
                                     : p.radar[(((size_t)b * 3 + (c - g.Cimg)) * g.Hr + (yy >> 2)) * g.Wr + (xx >> 2)];
#pragma unroll
          for (int n = 0; n < COUT; ++n) acc[n] = fmaf(v, wt[c * COUT + n], acc[n]);
        }
      }
    }
  }
  f32x4* zp = reinterpret_cast<f32x4*>(p.z + ((size_t)row * g.Wo + xo) * COUT);
#pragma unroll
  for (int n4 = 0; n4 < COUT / 4; ++n4) {
    const f32x4 o = {acc[4 * n4], acc[4 * n4 + 1], acc[4 * n4 + 2], acc[4 * n4 + 3]};
    zp[n4] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// input gradient (3x3, 16 input channels)
struct SdArgs {
  const float* gz;
  const float* weight;   // raw (Cout, 16, 3, 3)
  float* gx;
  SGeo g;
};

// gx[p, c] = sum over the taps and n of gz[(p + pad - tap) / stride, n] w[n, c, tap], the taps in row-major order, n ascending.
template <int COUT>
__global__ __launch_bounds__(256) void stem_conv_bwd_data_kernel(const SdArgs p) {
  __shared__ float wl[9 * COUT * 16];              // [tap][n][c]
  const SGeo& g = p.g;
  const int tid = threadIdx.x, s = g.stride;
  for (int i = tid; i < 9 * COUT * 16; i += 256) {
    const int c = i & 15, rest = i >> 4, n = rest % COUT, tap = rest / COUT;
    wl[i] = p.weight[((size_t)n * 16 + c) * 9 + tap];
  }
  __syncthreads();
  const int py = blockIdx.z / s, px = blockIdx.z - py * s;
  const int Hc = (g.H - py + s - 1) / s, Wc = (g.W - px + s - 1) / s;      // rows y = py + s yc < H of this parity, columns likewise
  const int xc = blockIdx.y * ST_COLS + (tid & 63);
  const long row = (long)blockIdx.x * ST_ROWS + (tid >> 6);               // over B * Hc
  if (xc >= Wc || row >= (long)g.B * Hc) return;
  const int b = (int)(row / Hc), yc = (int)(row - (long)b * Hc);
  const int y = py + s * yc, x = px + s * xc;
  const int t0y = (py + g.pad) % s, t0x = (px + g.pad) % s;                // first tap with (y + pad - ti) % stride == 0
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.0f;
  for (int ti = t0y; ti < 3; ti += s) {
    const int ny = y + g.pad - ti;
    if (ny < 0 || ny / s >= g.Ho) continue;
    for (int tj = t0x; tj < 3; tj += s) {
      const int nx = x + g.pad - tj;
      if (nx < 0 || nx / s >= g.Wo) continue;
      const f32x4* gp = reinterpret_cast<const f32x4*>(p.gz + (((size_t)b * g.Ho + ny / s) * g.Wo + nx / s) * COUT);
      const float* wt = wl + (ti * 3 + tj) * COUT * 16;
#pragma unroll
      for (int n4 = 0; n4 < COUT / 4; ++n4) {
        const f32x4 v = gp[n4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < 16; ++c) acc[c] = fmaf(v[e], wt[(n4 * 4 + e) * 16 + c], acc[c]);
      }
    }
  }
  f32x4* op = reinterpret_cast<f32x4*>(p.gx + (((size_t)b * g.H + y) * g.W + x) * 16);
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    const f32x4 o = {acc[4 * c4], acc[4 * c4 + 1], acc[4 * c4 + 2], acc[4 * c4 + 3]};
    op[c4] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// weight gradient
struct SwArgs {
  const float* gz;
  const float* x;
  const float* radar;
  float* ws;             // [slabs][Cout][k*k*Cin] partial gw, column = tap * Cin + c
  SGeo g;
  int nhwc;
  int ncol, ntiles;      // k*k*Cin and its 16-column tiles
  long M, slab_px;       // output pixels, pixels per slab (a multiple of 4)
};

constexpr int SW_CT = 3;   // column tiles per wave
constexpr int SW_U = 4;    // four-pixel steps per trip: every load ahead of the MFMAs

// One wave = one (slab of output pixels, group of three 16-column tiles, every 16-output tile): D[n, col] += gz[pix, n] patch[pix, col]
// with col = tap * Cin + c, four pixels per v_mfma_f32_16x16x4_f32; the halo is zero.  A lane's pixels advance by sixteen per
// trip, so their coordinates are stepped, not divided out (conv_bwd_weight_kernel's scheme).
template <int NT>
__global__ __launch_bounds__(64) void stem_conv_bwd_weight_kernel(const SwArgs p) {
  const SGeo& g = p.g;
  const int lane = threadIdx.x, kq = lane >> 4, cl = lane & 15;
  const long slab = blockIdx.x;
  const int grp = blockIdx.y;
  bool tv[SW_CT], cv[SW_CT];
  int cti[SW_CT], ctj[SW_CT], cc[SW_CT];
  const float* src[SW_CT];
#pragma unroll
  for (int t = 0; t < SW_CT; ++t) {
    const int tile = grp * SW_CT + t, col = tile * 16 + cl;
    tv[t] = tile < p.ntiles;                       // (wave-uniform)
    cv[t] = col < p.ncol;
    const int colc = cv[t] ? col : 0, tap = colc / g.Cin;
    cc[t] = colc - tap * g.Cin;
    cti[t] = tap / g.k;
    ctj[t] = tap - cti[t] * g.k;
    src[t] = cc[t] < g.Cimg ? p.x : p.radar;
  }
  const long HWo = (long)g.Ho * g.Wo;
  const long mb = slab * p.slab_px, me = mb + p.slab_px < p.M ? mb + p.slab_px : p.M;
  int pb[SW_U], ph[SW_U], pw[SW_U];                // image, row, column of this lane's pixel of step u
#pragma unroll
  for (int u = 0; u < SW_U; ++u) {
    const long m = mb + 4 * u + kq;
    pb[u] = (int)(m / HWo);
    const long rem = m - pb[u] * HWo;
    ph[u] = (int)(rem / g.Wo);
    pw[u] = (int)(rem - (long)ph[u] * g.Wo);
  }
  f32x4 acc[NT][SW_CT];
#pragma unroll
  for (int r = 0; r < NT; ++r)
#pragma unroll
    for (int t = 0; t < SW_CT; ++t) acc[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long m4 = mb; m4 < me; m4 += 4 * SW_U) {
    float a[SW_U][NT], xv[SW_U][SW_CT];
#pragma unroll
    for (int u = 0; u < SW_U; ++u) {
      const long m = m4 + 4 * u + kq;
      const bool live = m < me;
      const size_t gi = live ? (size_t)m * g.Cout : 0;                      // (every lane loads from a valid address; the select drops it)
#pragma unroll
      for (int r = 0; r < NT; ++r) {
        const float gv = p.gz[gi + r * 16 + cl];
        a[u][r] = live ? gv : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < SW_CT; ++t) {
        xv[u][t] = 0.0f;
        if (tv[t]) {
          const int yy = ph[u] * g.stride - g.pad + cti[t], xx = pw[u] * g.stride - g.pad + ctj[t];
          const bool in = live && cv[t] && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
          size_t xi = 0;
          if (in) {
            if (p.nhwc) xi = (((size_t)pb[u] * g.H + yy) * g.W + xx) * g.Cin + cc[t];
            else if (cc[t] < g.Cimg) xi = (((size_t)pb[u] * g.Cimg + cc[t]) * g.H + yy) * g.W + xx;
            else xi = (((size_t)pb[u] * 3 + (cc[t] - g.Cimg)) * g.Hr + (yy >> 2)) * g.Wr + (xx >> 2);
          }
          const float v = src[t][xi];
          xv[u][t] = in ? v : 0.0f;
        }
      }
      pw[u] += 4 * SW_U;
      while (pw[u] >= g.Wo) {
        pw[u] -= g.Wo;
        if (++ph[u] == g.Ho) {
          ph[u] = 0;
          ++pb[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SW_U; ++u)
#pragma unroll
      for (int r = 0; r < NT; ++r)
#pragma unroll
        for (int t = 0; t < SW_CT; ++t)
          if (tv[t]) acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][r], xv[u][t], acc[r][t], 0, 0, 0);
  }
  float* wsp = p.ws + (size_t)slab * g.Cout * p.ncol;
#pragma unroll
  for (int r = 0; r < NT; ++r)
#pragma unroll
    for (int t = 0; t < SW_CT; ++t) {
      const int col = (grp * SW_CT + t) * 16 + cl;
      if (tv[t] && cv[t]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) wsp[(size_t)(r * 16 + kq * 4 + j) * p.ncol + col] = acc[r][t][j];
      }
    }
}

// gw[n][c][tap] = sum over the slabs, in slab order, of ws[slab][n][tap * Cin + c]
__global__ __launch_bounds__(256) void stem_conv_bwd_reduce_kernel(const float* __restrict__ ws, int slabs, int Cout, int Cin, int kk,
                                                                   float* __restrict__ gw) {
  const int ncol = kk * Cin, per = Cout * ncol;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < per; j += gridDim.x * 256) {
    float v = ws[j];
    for (int z = 1; z < slabs; ++z) v += ws[(size_t)z * per + j];
    const int n = j / ncol, col = j - n * ncol, tap = col / Cin, c = col - tap * Cin;
    gw[((size_t)n * Cin + c) * kk + tap] = v;
  }
}

// slabs of output pixels and their length (functions of the geometry alone): at least 256 pixels each, about 2048 waves at the
// most, a multiple of four pixels per slab (four pixels per MFMA), no empty slab
void sw_slabs(long M, int ncol, int* slabs, long* slab_px) {
  const int ntiles = (ncol + 15) / 16, groups = (ntiles + SW_CT - 1) / SW_CT;
  long s = (M + 255) / 256;
  const long cap = 2048 / groups > 1 ? 2048 / groups : 1;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  long px = (M + s - 1) / s;
  px = (px + 3) & ~3L;
  *slab_px = px;
  *slabs = (int)((M + px - 1) / px);
}

}  // namespace

extern "C" size_t cf_stem_conv_bwd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || (Cout != 16 && Cout != 32) || stride < 1 || stride > 2) return 0;
  if (!((k == 7 && stride == 1 && Cin > 0 && Cin <= 8) || (k == 3 && Cin == 16))) return 0;
  const int pad = (k - 1) / 2;
  const long M = (long)B * ((H + 2 * pad - k) / stride + 1) * ((W + 2 * pad - k) / stride + 1);
  int slabs;
  long px;
  sw_slabs(M, k * k * Cin, &slabs, &px);
  return (size_t)slabs * Cout * k * k * Cin * sizeof(float);
}

extern "C" int cf_stem_conv_forward(const float* x, const float* radar, const float* weight, int B, int H, int W, int Cin, int Cout,
                                    int k, int stride, float* z, void* stream) {
  SfArgs a{};
  if (int e = sgeo_check("cf_stem_conv_forward", B, H, W, Cin, Cout, k, stride, radar != nullptr, &a.g)) return e;
  CF_REQUIRE(x && weight && z, "cf_stem_conv_forward: null buffer");
  CF_REQUIRE(al16(z) && (k == 7 || al16(x)), "cf_stem_conv_forward: NHWC buffers must be 16-byte aligned");
  a.x = x; a.radar = radar; a.weight = weight; a.z = z;
  const long rows = (long)B * a.g.Ho;
  const dim3 grid((unsigned)((rows + ST_ROWS - 1) / ST_ROWS), (unsigned)((a.g.Wo + ST_COLS - 1) / ST_COLS));
  CF_REQUIRE(grid.y < 65536, "cf_stem_conv_forward: map too wide for the launch grid");
  const size_t lds = (size_t)k * k * Cin * Cout * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (k == 7) {
    if (Cout == 16) hipLaunchKernelGGL((stem_conv_fwd_kernel<16, false>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((stem_conv_fwd_kernel<32, false>), grid, dim3(256), lds, st, a);
  } else {
    if (Cout == 16) hipLaunchKernelGGL((stem_conv_fwd_kernel<16, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((stem_conv_fwd_kernel<32, true>), grid, dim3(256), lds, st, a);
  }
  return cf_check_launch("cf_stem_conv_forward");
}

extern "C" int cf_stem_conv_bwd_weight(const float* gz, const float* x, const float* radar, int B, int H, int W, int Cin, int Cout,
                                       int k, int stride, float* gw, void* workspace, size_t workspace_bytes, void* stream) {
  SwArgs a{};
  if (int e = sgeo_check("cf_stem_conv_bwd_weight", B, H, W, Cin, Cout, k, stride, radar != nullptr, &a.g)) return e;
  CF_REQUIRE(gz && x && gw, "cf_stem_conv_bwd_weight: null buffer");
  CF_REQUIRE(workspace && workspace_bytes >= cf_stem_conv_bwd_workspace_bytes(B, H, W, Cin, Cout, k, stride),
             "cf_stem_conv_bwd_weight: workspace of %zu bytes is smaller than cf_stem_conv_bwd_workspace_bytes(...)", workspace_bytes);
  a.gz = gz; a.x = x; a.radar = radar ? radar : x; a.ws = static_cast<float*>(workspace);
  a.nhwc = k == 3;
  a.ncol = k * k * Cin;
  a.ntiles = (a.ncol + 15) / 16;
  a.M = (long)B * a.g.Ho * a.g.Wo;
  int slabs;
  sw_slabs(a.M, a.ncol, &slabs, &a.slab_px);
  const dim3 grid((unsigned)slabs, (unsigned)((a.ntiles + SW_CT - 1) / SW_CT));
  hipStream_t st = (hipStream_t)stream;
  if (Cout == 16) hipLaunchKernelGGL(stem_conv_bwd_weight_kernel<1>, grid, dim3(64), 0, st, a);
  else hipLaunchKernelGGL(stem_conv_bwd_weight_kernel<2>, grid, dim3(64), 0, st, a);
  const int total = Cout * a.ncol;
  hipLaunchKernelGGL(stem_conv_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.ws, slabs, Cout, Cin, k * k,
                     gw);
  return cf_check_launch("cf_stem_conv_bwd_weight");
}

extern "C" int cf_stem_conv_bwd_data(const float* gz, const float* weight, int B, int H, int W, int Cin, int Cout, int k, int stride,
                                     float* gx, void* stream) {
  SdArgs a{};
  if (int e = sgeo_check("cf_stem_conv_bwd_data", B, H, W, Cin, Cout, k, stride, false, &a.g)) return e;
  CF_REQUIRE(k == 3, "cf_stem_conv_bwd_data: k=%d - only the 3x3 layers have an input gradient (nothing differentiates the image)", k);
  CF_REQUIRE(gz && weight && gx, "cf_stem_conv_bwd_data: null buffer");
  CF_REQUIRE(al16(gz) && al16(gx), "cf_stem_conv_bwd_data: buffers must be 16-byte aligned");
  a.gz = gz; a.weight = weight; a.gx = gx;
  const long rows = (long)B * ((H + stride - 1) / stride);                  // the largest parity class
  const int cols = (W + stride - 1) / stride;
  const dim3 grid((unsigned)((rows + ST_ROWS - 1) / ST_ROWS), (unsigned)((cols + ST_COLS - 1) / ST_COLS), (unsigned)(stride * stride));
  CF_REQUIRE(grid.y < 65536, "cf_stem_conv_bwd_data: map too wide for the launch grid");
  hipStream_t st = (hipStream_t)stream;
  if (Cout == 16) hipLaunchKernelGGL(stem_conv_bwd_data_kernel<16>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(stem_conv_bwd_data_kernel<32>, grid, dim3(256), 0, st, a);
  return cf_check_launch("cf_stem_conv_bwd_data");
}
