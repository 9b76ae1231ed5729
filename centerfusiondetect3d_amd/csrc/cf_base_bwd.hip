// Training kernels of the DLA-34 base, levels 2-5 (ops.conv_bn_act / ops.max_pool2x2), fp32 NHWC.  One block shape covers the
// levels: convolution (3x3 stride 1 or 2, or 1x1, no bias) -> BatchNorm -> [+ residual] -> [ReLU].
//
//   cf_conv_bwd_weight        gw (N,C,k,k) from gz and the block input: slab partials, added in slab order by a second launch
//   cf_conv_bwd_data          gx from gz and the raw weight (N,C,k,k): plain stores, every pixel row owned by one workgroup
//   cf_bn_act_train_forward   y = act(bn(x) [+ residual]); statistics, running statistics and workspace of cf_bn_relu_train_forward
//   cf_bn_act_backward        gz, gres, ggamma, gbeta; the ReLU mask recomputed from the forward's expression, residual included
//   cf_maxpool2x2_bwd         the whole gradient to the first maximum of each 2x2 window in row-major order (aten's rule)
//
// Geometry of the two convolution kernels: k = 1 or 3, padding (k - 1) / 2, stride 1 or 2 (2 with k = 3 only),
// Ho = (H + 2 pad - k) / stride + 1; C and N multiples of 32, C <= 1280, N <= 512.  Products go through the exact fp32-input
// v_mfma_f32_32x32x2_f32: no range to guard.  No float atomics in this file: every result is bitwise reproducible.
#include "cf_bn_train.h"

namespace {

struct Geo {
  int B, H, W, C, N, Ho, Wo, k, stride, pad;
};

int geo_check(const char* who, int B, int H, int W, int C, int N, int k, int stride, Geo* g) {
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  CF_REQUIRE((k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)),
             "%s: k=%d stride=%d (1x1 stride 1, or 3x3 stride 1 or 2)", who, k, stride);
  CF_REQUIRE(C > 0 && C % 32 == 0 && C <= 1280, "%s: C=%d must be a multiple of 32, at most 1280", who, C);
  CF_REQUIRE(N > 0 && N % 32 == 0 && N <= 512, "%s: N=%d must be a multiple of 32, at most 512", who, N);
  g->B = B; g->H = H; g->W = W; g->C = C; g->N = N; g->k = k; g->stride = stride;
  g->pad = (k - 1) / 2;
  g->Ho = (H + 2 * g->pad - k) / stride + 1;
  g->Wo = (W + 2 * g->pad - k) / stride + 1;
  CF_REQUIRE((long)B * H * W * C < (1L << 31) && (long)B * g->Ho * g->Wo * N < (1L << 31), "%s: tensor too large", who);
  return CF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// weight gradient
struct BwArgs {
  const float* gz;
  const float* x;
  float* ws;        // [slabs][k*k][N][C] partial gw
  Geo g;
  int M;            // output pixels
  int slab_px;
};

constexpr int BW_PAIRS = 4;   // pixel pairs per trip: every load ahead of the MFMAs

// One wave = one (slab of output pixels, tap, two 32-output tiles, two 32-channel chunks): D[n, c] += gz[pix, n] x[pix * stride + tap, c],
// two pixels per MFMA, four MFMAs per four operand loads; the halo is zero.  (conv3x3_bwd_weight_kernel's tiling with N in
// 32-wide tiles and a stride; a lane's pixels advance by eight per trip, so their coordinates are stepped, not divided out.)
__global__ __launch_bounds__(64) void conv_bwd_weight_kernel(const BwArgs p) {
  const Geo& g = p.g;
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int slab = blockIdx.x;
  const int nch = g.C >> 5, nnt = g.N >> 5;
  const int gch = (nch + 1) >> 1, gnt = (nnt + 1) >> 1;
  const int tap = blockIdx.y / (gch * gnt), rest = blockIdx.y - tap * gch * gnt;
  const int ntp = rest / gch, chp = rest - ntp * gch;
  const bool n_two = 2 * ntp + 1 < nnt, c_two = 2 * chp + 1 < nch;         // (wave-uniform: an odd tile count leaves one single)
  const int nt0 = 2 * ntp, nt1 = n_two ? nt0 + 1 : nt0, ch0 = 2 * chp, ch1 = c_two ? ch0 + 1 : ch0;
  const int n0 = nt0 * 32 + cl, n1 = nt1 * 32 + cl, c0 = ch0 * 32 + cl, c1 = ch1 * 32 + cl;
  const int ti = tap / g.k, tj = tap - ti * g.k;
  const int HWo = g.Ho * g.Wo;
  const int mb = slab * p.slab_px, me = min(mb + p.slab_px, p.M);
  int pb[BW_PAIRS], ph[BW_PAIRS], pw[BW_PAIRS];                            // image, row, column of this lane's pixel of pair u
#pragma unroll
  for (int u = 0; u < BW_PAIRS; ++u) {
    const int m = mb + 2 * u + half;
    pb[u] = m / HWo;
    const int rem = m - pb[u] * HWo;
    ph[u] = rem / g.Wo;
    pw[u] = rem - ph[u] * g.Wo;
  }
  f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc00[r] = acc01[r] = acc10[r] = acc11[r] = 0.0f;
  for (int m2 = mb; m2 < me; m2 += 2 * BW_PAIRS) {
    float a0[BW_PAIRS], a1[BW_PAIRS], x0[BW_PAIRS], x1[BW_PAIRS];
#pragma unroll
    for (int u = 0; u < BW_PAIRS; ++u) {
      const bool live = m2 + 2 * u + half < me;
      const size_t gi = live ? (size_t)(m2 + 2 * u + half) * g.N : 0;      // (every lane loads from a valid address; the select drops it)
      const float g0 = p.gz[gi + n0], g1 = p.gz[gi + n1];
      a0[u] = live ? g0 : 0.0f;
      a1[u] = live ? g1 : 0.0f;
      const int yy = ph[u] * g.stride - g.pad + ti, xx = pw[u] * g.stride - g.pad + tj;
      const bool in = live && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
      const size_t xi = in ? ((size_t)(pb[u] * g.H + yy) * g.W + xx) * g.C : 0;
      const float v0 = p.x[xi + c0], v1 = p.x[xi + c1];
      x0[u] = in ? v0 : 0.0f;
      x1[u] = in ? v1 : 0.0f;
      pw[u] += 2 * BW_PAIRS;
      while (pw[u] >= g.Wo) {
        pw[u] -= g.Wo;
        if (++ph[u] == g.Ho) {
          ph[u] = 0;
          ++pb[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < BW_PAIRS; ++u) {
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], x0[u], acc00, 0, 0, 0);
      if (c_two) acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], x1[u], acc01, 0, 0, 0);
      if (n_two) acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], x0[u], acc10, 0, 0, 0);
      if (n_two && c_two) acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], x1[u], acc11, 0, 0, 0);
    }
  }
  float* wsp = p.ws + ((size_t)slab * g.k * g.k + tap) * g.N * g.C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = (r & 3) + 8 * (r >> 2) + 4 * half;
    wsp[(size_t)(nt0 * 32 + o) * g.C + c0] = acc00[r];
    if (c_two) wsp[(size_t)(nt0 * 32 + o) * g.C + c1] = acc01[r];
    if (n_two) wsp[(size_t)(nt1 * 32 + o) * g.C + c0] = acc10[r];
    if (n_two && c_two) wsp[(size_t)(nt1 * 32 + o) * g.C + c1] = acc11[r];
  }
}

// gw[n][c][tap] = sum over the slabs, in slab order, of ws[slab][tap][n][c]
__global__ __launch_bounds__(256) void conv_bwd_reduce_kernel(const float* __restrict__ ws, int slabs, int kk, long NC,
                                                              float* __restrict__ gw) {
  const long per = (long)kk * NC;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < per; j += (long)gridDim.x * 256) {
    float v = ws[j];
    for (int z = 1; z < slabs; ++z) v += ws[(size_t)z * per + j];
    const int tap = (int)(j / NC);
    const long nc = j - (long)tap * NC;
    gw[nc * kk + tap] = v;
  }
}

// slabs of output pixels (a function of the geometry alone): at least 256 pixels each, about 2048 waves of up to four tiles at the most
int bw_slabs(long M, int C, int N, int k) {
  const long per_slab = (long)k * k * ((C / 32 + 1) / 2) * ((N / 32 + 1) / 2);
  long s = (M + 255) / 256;
  const long cap = 2048 / per_slab > 1 ? 2048 / per_slab : 1;
  if (s > cap) s = cap;
  return (int)(s < 1 ? 1 : s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// input gradient
struct BdArgs {
  const float* gz;
  const float* weight;   // raw (N, C, k, k)
  float* gx;
  Geo g;
};

constexpr int BD_PX = 32;   // input pixels per workgroup: one 32x32 MFMA tile per wave, each wave its own 32-channel chunk

// gx[p, c] = sum over the taps and n of gz[(p + pad - tap) / stride, n] w[n, c, tap].  Under stride 2 a workgroup's 32 pixels
// share the parity of their row and of their column (blockIdx.z), so the tap loop walks the taps of that parity alone: 1, 2, 2
// or 4 of the 9.  Per 32 outputs the shifted gz tiles are staged once in A-operand order; a pixel row of gx belongs to this
// workgroup alone (and a 32-channel chunk of it to one wave).
__global__ __launch_bounds__(256) void conv_bwd_data_kernel(const BdArgs p) {
  __shared__ float afrag[9 * 16 * 64];             // [tap slot][k-step][lane]: pixel l & 31, output 2 s + (l >> 5)
  __shared__ int srcq[9 * BD_PX];                  // [tap slot][pixel]: the gz pixel that tap reads, -1 outside the map
  __shared__ int pixq[BD_PX];                      // the gx pixel, -1 behind the end
  const Geo& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  const int s = g.stride, kk = g.k * g.k;
  const int py = blockIdx.z / s, px = blockIdx.z - py * s;
  const int Hc = (g.H - py + s - 1) / s, Wc = (g.W - px + s - 1) / s;      // rows y = py + s yc < H of this parity, columns likewise
  const int Mc = g.B * Hc * Wc;
  const int m0 = blockIdx.x * BD_PX;
  if (m0 >= Mc) return;
  const int t0y = (py + g.pad) % s, t0x = (px + g.pad) % s;                // first tap with (y + pad - ti) % stride == 0
  const int nty = (g.k - t0y + s - 1) / s, ntx = (g.k - t0x + s - 1) / s;
  const int ntaps = nty * ntx;
  for (int i = tid; i < ntaps * BD_PX; i += nt) {
    const int slot = i >> 5, j = i & 31, m = m0 + j;
    int q = -1, pq = -1;
    if (m < Mc) {
      const int b = m / (Hc * Wc), rem = m - b * Hc * Wc;
      const int yc = rem / Wc, xc = rem - yc * Wc;
      const int y = py + s * yc, x = px + s * xc;
      const int sy = slot / ntx, sx = slot - sy * ntx;
      const int ny = y + g.pad - (t0y + s * sy), nx = x + g.pad - (t0x + s * sx);
      const int qy = ny / s, qx = nx / s;
      if (ny >= 0 && nx >= 0 && qy < g.Ho && qx < g.Wo) q = (b * g.Ho + qy) * g.Wo + qx;
      pq = (b * g.H + y) * g.W + x;
    }
    srcq[i] = q;
    if (slot == 0) pixq[j] = pq;
  }
  const int half = lane >> 5, cl = lane & 31;
  const int nch = g.C >> 5;
  const int ch = blockIdx.y * nw + wave;
  const int c = min(ch, nch - 1) * 32 + cl;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int n0 = 0; n0 < g.N; n0 += 32) {
    __syncthreads();                               // (the index tables are written; the previous chunk's tiles are read)
    for (int i = tid; i < ntaps * 16 * 64; i += nt) {
      const int slot = i >> 10, st = (i >> 6) & 15, l = i & 63;
      const int q = srcq[slot * BD_PX + (l & 31)];
      const float v = p.gz[(size_t)max(q, 0) * g.N + n0 + 2 * st + (l >> 5)];
      afrag[i] = q >= 0 ? v : 0.0f;
    }
    __syncthreads();
    if (ch >= nch) continue;
    for (int slot = 0; slot < ntaps; ++slot) {
      const int sy = slot / ntx, sx = slot - sy * ntx;
      const int tap = (t0y + s * sy) * g.k + t0x + s * sx;
      const float* wp = p.weight + ((size_t)n0 * g.C + c) * kk + tap;
      for (int s0 = 0; s0 < 16; s0 += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int st = s0 + u;
          bv[u] = wp[(size_t)(2 * st + half) * g.C * kk];
          av[u] = afrag[(slot * 16 + st) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);         // (all eight steps' loads ahead of their MFMAs)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      }
    }
  }
  if (ch >= nch) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int pq = pixq[(r & 3) + 8 * (r >> 2) + 4 * half];
    if (pq >= 0) p.gx[(size_t)pq * g.C + c] = acc[r];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2x2 max-pool backward: one thread per window and 16-byte channel group.  The rows / columns an odd H / W leaves behind the
// last window get zeros.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ x,
                                                             float* __restrict__ gx, int H, int W, int C4) {
  const int Ho = H / 2, Wo = W / 2, Ww = (W + 1) / 2;
  const int yo = blockIdx.y, b = blockIdx.z;
  const int y0 = 2 * yo;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  f32x4* g4 = reinterpret_cast<f32x4*>(gx);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int j = blockIdx.x * 256 + threadIdx.x; j < Ww * C4; j += gridDim.x * 256) {
    const int xo = j / C4, c4 = j - xo * C4;
    const int x0 = 2 * xo;
    const size_t i00 = ((size_t)(b * H + y0) * W + x0) * C4 + c4;
    const size_t off[4] = {i00, i00 + C4, i00 + (size_t)W * C4, i00 + (size_t)W * C4 + C4};
    if (yo < Ho && xo < Wo) {
      const f32x4 go = reinterpret_cast<const f32x4*>(gout)[((size_t)(b * Ho + yo) * Wo + xo) * C4 + c4];
      f32x4 v[4], o[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = x4[off[t]];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float best = -INFINITY;
        int idx = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (v[t][e] > best || v[t][e] != v[t][e]) {       // (aten: a later value wins only if greater, or NaN)
            best = v[t][e];
            idx = t;
          }
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t][e] = idx == t ? go[e] : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) g4[off[t]] = o[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (y0 + (t >> 1) < H && x0 + (t & 1) < W) g4[off[t]] = zero;
    }
  }
}

}  // namespace

extern "C" size_t cf_conv_bwd_workspace_bytes(int B, int H, int W, int C, int N, int k, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0 || C % 32 || N % 32 || (k != 1 && k != 3) || stride < 1 || stride > 2) return 0;
  const int pad = (k - 1) / 2;
  const long M = (long)B * ((H + 2 * pad - k) / stride + 1) * ((W + 2 * pad - k) / stride + 1);
  return (size_t)bw_slabs(M, C, N, k) * k * k * N * C * sizeof(float);
}

extern "C" int cf_conv_bwd_weight(const float* gz, const float* x, int B, int H, int W, int C, int N, int k, int stride, float* gw,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  BwArgs a{};
  if (int e = geo_check("cf_conv_bwd_weight", B, H, W, C, N, k, stride, &a.g)) return e;
  CF_REQUIRE(gz && x && gw, "cf_conv_bwd_weight: null buffer");
  CF_REQUIRE(workspace && workspace_bytes >= cf_conv_bwd_workspace_bytes(B, H, W, C, N, k, stride),
             "cf_conv_bwd_weight: workspace of %zu bytes is smaller than cf_conv_bwd_workspace_bytes(...)", workspace_bytes);
  const long M = (long)B * a.g.Ho * a.g.Wo;
  const int slabs = bw_slabs(M, C, N, k);
  a.gz = gz; a.x = x; a.ws = static_cast<float*>(workspace);
  a.M = (int)M;
  a.slab_px = (int)((M + slabs - 1) / slabs);
  a.slab_px += a.slab_px & 1;                       // (two pixels per MFMA: slabs start on an even pixel)
  hipStream_t st = (hipStream_t)stream;
  const int kk = k * k;
  hipLaunchKernelGGL(conv_bwd_weight_kernel, dim3((unsigned)slabs, (unsigned)(kk * ((C / 32 + 1) / 2) * ((N / 32 + 1) / 2))), dim3(64), 0,
                     st, a);
  const long total = (long)kk * N * C;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, a.ws, slabs, kk,
                     (long)N * C, gw);
  return cf_check_launch("cf_conv_bwd_weight");
}

extern "C" int cf_conv_bwd_data(const float* gz, const float* weight, int B, int H, int W, int C, int N, int k, int stride, float* gx,
                                void* stream) {
  BdArgs a{};
  if (int e = geo_check("cf_conv_bwd_data", B, H, W, C, N, k, stride, &a.g)) return e;
  CF_REQUIRE(gz && weight && gx, "cf_conv_bwd_data: null buffer");
  a.gz = gz; a.weight = weight; a.gx = gx;
  const int nch = C / 32;
  const unsigned waves = (unsigned)(nch < 4 ? nch : 4);
  const long mc = (long)B * ((H + stride - 1) / stride) * ((W + stride - 1) / stride);      // the largest parity class
  hipLaunchKernelGGL(conv_bwd_data_kernel, dim3((unsigned)((mc + BD_PX - 1) / BD_PX), (unsigned)((nch + waves - 1) / waves),
                                                (unsigned)(stride * stride)),
                     dim3(64 * waves), 0, (hipStream_t)stream, a);
  return cf_check_launch("cf_conv_bwd_data");
}

extern "C" size_t cf_bn_act_workspace_bytes(long M, int C) { return bn_workspace_bytes(M, C); }

extern "C" int cf_bn_act_train_forward(const float* x, const float* gamma, const float* beta, const float* residual, int relu,
                                       float* running_mean, float* running_var, int training, float momentum, float eps, long M, int C,
                                       float* y, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return bn_train_forward("cf_bn_act_train_forward", x, gamma, beta, residual, relu != 0, running_mean, running_var, training, momentum,
                          eps, M, C, y, save_mean, save_invstd, workspace, workspace_bytes, stream);
}

extern "C" int cf_bn_act_backward(const float* gy, const float* x, const float* gamma, const float* beta, const float* residual, int relu,
                                  const float* save_mean, const float* save_invstd, int training, long M, int C, float* gz, float* gres,
                                  float* ggamma, float* gbeta, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_train_backward("cf_bn_act_backward", gy, x, gamma, beta, residual, relu != 0, save_mean, save_invstd, training, M, C, gz,
                           gres, ggamma, gbeta, workspace, workspace_bytes, stream);
}

extern "C" int cf_maxpool2x2_bwd(const float* gout, const float* x, int B, int H, int W, int C, float* gx, void* stream) {
  CF_REQUIRE(gout && x && gx, "cf_maxpool2x2_bwd: null buffer");
  CF_REQUIRE(B > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "cf_maxpool2x2_bwd: bad geometry");
  CF_REQUIRE((H + 1) / 2 < 65536 && B < 65536, "cf_maxpool2x2_bwd: too many rows / images for the launch grid");
  CF_REQUIRE(aligned16({gout, x, gx}), "cf_maxpool2x2_bwd: buffers must be 16-byte aligned");
  CF_REQUIRE((long)B * H * W * C < (1L << 40), "cf_maxpool2x2_bwd: tensor too large");
  const int row_len = ((W + 1) / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3((unsigned)((row_len + 255) / 256), (unsigned)((H + 1) / 2), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, gout, x, gx, H, W, C / 4);
  return cf_check_launch("cf_maxpool2x2_bwd");
}
