// Training kernels of the neck's DeformConv block and IDA upsample (ops.deform_conv_block / ops.upsample_dw_add), fp32 NHWC:
//
//   cf_offmask_activate       sigmoid of the mask logits in the offset convolution's output, in place
//   cf_conv3x3_bwd_weight     gw (27,C,3,3) / gbias (27) of conv_offset_mask from the DCN backward's gom and the block input
//   cf_conv3x3_bwd_data       gx += conv_offset_mask's input gradient (plain read-modify-write behind the DCN's atomics)
//   cf_bn_relu_train_forward  batch statistics (slab-local two-pass, slabs merged in float64), running statistics, y = relu(bn(x))
//   cf_bn_relu_backward       gz, ggamma, gbeta from gy and the saved pre-BN map
//   cf_upsample_dw_bwd        gx / gweight of cf_upsample_dw
//
// The BatchNorm kernels and the column-reduction helpers live in cf_bn_train.h, shared with cf_base_bwd.hip (cf_bn_act_*).
// The two convolution kernels read gom with the mask derivative folded in on load: channels 18..26 of gom are the gradient with
// respect to the ACTIVATED mask m (saved in offmask), the convolution produced its logit, so they are multiplied by m (1 - m).
// Products that go through MFMA use the exact fp32-input v_mfma_f32_32x32x2_f32.  Every parameter gradient is a sum of slab
// partials added in slab order by a second launch: bitwise reproducible, no float atomics anywhere in this file.
#include "cf_bn_train.h"

namespace {

constexpr int OMC = 32;   // floats per pixel of offmask / gom
constexpr int OMN = 27;   // channels the offset convolution produces

__device__ __forceinline__ float fold_mask(float g, float om, int n) {
  return n < 18 ? g : (n < OMN ? g * (om * (1.0f - om)) : 0.0f);
}

// channels 18..26 of an offmask buffer, in place: mask logits -> the activated mask (what the backward kernels and the DCN with
// mask_activated read).  One pixel per thread, its channels 16..27 as three 16-byte vectors.
__global__ __launch_bounds__(256) void offmask_activate_kernel(float* __restrict__ om, long M) {
  for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
    f32x4* row = reinterpret_cast<f32x4*>(om + m * OMC) + 4;
    f32x4 a = row[0], b = row[1], c = row[2];
    a[2] = cf_sigmoid(a[2]);
    a[3] = cf_sigmoid(a[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = cf_sigmoid(b[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) c[e] = cf_sigmoid(c[e]);
    row[0] = a;
    row[1] = b;
    row[2] = c;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// offset convolution: weight gradient
struct CwArgs {
  const float* gom;
  const float* om;
  const float* x;
  float* ws;        // [slabs][9][27][C] partial gw, then [slabs][27] partial gbias
  int H, W, C, M;
  int slab_px;
  int want_gw;
};

constexpr int CW_PAIRS = 4;   // pixel pairs per trip (as the DCN weight kernel: every load ahead of the MFMAs)

// One wave = one (pixel slab, tap, 32-channel chunk): D[n, c] += gom'[pix, n] x[pix + tap, c], two pixels per MFMA; the halo is zero.
__global__ __launch_bounds__(64) void conv3x3_bwd_weight_kernel(const CwArgs p) {
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int slab = blockIdx.x;
  const int nch = p.C >> 5;
  const int tap = blockIdx.y / nch, ch = blockIdx.y - tap * nch;
  const int ti = tap / 3, tj = tap - ti * 3;
  const int HW = p.H * p.W;
  const int mb = slab * p.slab_px, me = min(mb + p.slab_px, p.M);
  const int c = ch * 32 + cl;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bsum = 0.0f;
  for (int m2 = mb; m2 < me; m2 += 2 * CW_PAIRS) {
    float a[CW_PAIRS], col[CW_PAIRS];
#pragma unroll
    for (int u = 0; u < CW_PAIRS; ++u) {
      const int m = m2 + 2 * u + half;
      const bool live = m < me;
      const int mc = live ? m : me - 1;
      const float g = p.gom[(size_t)mc * OMC + cl], o = p.om[(size_t)mc * OMC + cl];
      a[u] = live ? fold_mask(g, o, cl) : 0.0f;
      const int b = mc / HW, rem = mc - b * HW;
      const int ho = rem / p.W, wo = rem - ho * p.W;
      const int yy = ho - 1 + ti, xx = wo - 1 + tj;
      const bool in = live && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
      const int yc = min(max(yy, 0), p.H - 1), xc = min(max(xx, 0), p.W - 1);
      const float v = p.x[((size_t)(b * p.H + yc) * p.W + xc) * p.C + c];
      col[u] = in ? v : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < CW_PAIRS; ++u) bsum += a[u];
    if (!p.want_gw) continue;
#pragma unroll
    for (int u = 0; u < CW_PAIRS; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], col[u], acc, 0, 0, 0);
  }
  if (p.want_gw) {
    float* wsp = p.ws + ((size_t)slab * 9 + tap) * OMN * p.C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (o < OMN) wsp[(size_t)o * p.C + c] = acc[r];
    }
  }
  if (blockIdx.y == 0) {
    float* wsb = p.ws + (size_t)gridDim.x * 9 * OMN * p.C + (size_t)slab * OMN;
    const float v = bsum + __shfl_xor(bsum, 32, 64);     // (even pixels) + (odd pixels): one fixed order
    if (half == 0 && cl < OMN) wsb[cl] = v;
  }
}

// gw[n][c][k] = sum over the slabs, in slab order, of ws[slab][k][n][c]; gbias[n] likewise
__global__ __launch_bounds__(256) void conv3x3_bwd_reduce_kernel(const float* __restrict__ ws, int slabs, int C,
                                                                 float* __restrict__ gw, float* __restrict__ gbias) {
  const long per = (long)9 * OMN * C;
  const long total = (gw ? per : 0) + (gbias ? OMN : 0);
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total; j += (long)gridDim.x * 256) {
    if (gw && j < per) {
      float v = ws[j];
      for (int z = 1; z < slabs; ++z) v += ws[(size_t)z * per + j];
      const int k = (int)(j / ((long)OMN * C));
      const long oc = j - (long)k * OMN * C;
      gw[oc * 9 + k] = v;
    } else {
      const long o = j - (gw ? per : 0);
      const float* wb = ws + (size_t)slabs * per;
      float v = wb[o];
      for (int z = 1; z < slabs; ++z) v += wb[(size_t)z * OMN + o];
      gbias[o] = v;
    }
  }
}

// pixel slabs of the weight gradient (a function of the geometry alone): at least 256 pixels each, about 8192 waves at the most
// (one wave per workgroup and a latency-bound loop: eight waves per SIMD hide what two cannot)
int cw_slabs(long M, int C) {
  const long per_slab = 9L * (C / 32);
  long s = (M + 255) / 256;
  const long cap = 8192 / per_slab > 1 ? 8192 / per_slab : 1;
  if (s > cap) s = cap;
  return (int)(s < 1 ? 1 : s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// offset convolution: input gradient, added into gx
struct CdArgs {
  const float* gom;
  const float* om;
  const float* weight;   // raw (27, C, 3, 3)
  float* gx;
  int H, W, C, M;
};

constexpr int CD_PX = 32;   // pixels per workgroup: one 32x32 MFMA tile, its waves take the 32-channel chunks round robin

// gx[p, c] += sum over taps and n of gom'[p - tap, n] w[n, c, tap].  The nine shifted gom' tiles are staged once, in A-operand
// order; a pixel row of gx belongs to this workgroup alone (and a 32-channel chunk of it to one wave).
__global__ __launch_bounds__(256) void conv3x3_bwd_data_kernel(const CdArgs p) {
  __shared__ float afrag[9 * 16 * 64];             // [tap][k-step][lane]: pixel l & 31, channel 2 s + (l >> 5)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  const int m0 = blockIdx.x * CD_PX;
  const int HW = p.H * p.W;
  for (int i = tid; i < 9 * 16 * 64; i += nt) {
    const int tap = i >> 10, s = (i >> 6) & 15, l = i & 63;
    const int ti = tap / 3, tj = tap - ti * 3;
    const int n = 2 * s + (l >> 5), m = min(m0 + (l & 31), p.M - 1);
    const int b = m / HW, rem = m - b * HW;
    const int ho = rem / p.W, wo = rem - ho * p.W;
    const int yy = ho + 1 - ti, xx = wo + 1 - tj;
    const bool in = m0 + (l & 31) < p.M && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
    const int yc = min(max(yy, 0), p.H - 1), xc = min(max(xx, 0), p.W - 1);
    const size_t q = ((size_t)(b * p.H + yc) * p.W + xc) * OMC + n;
    const float g = p.gom[q], o = p.om[q];
    afrag[i] = in ? fold_mask(g, o, n) : 0.0f;
  }
  __syncthreads();
  const int half = lane >> 5, cl = lane & 31;
  const int nch = p.C >> 5;
  for (int ch = wave; ch < nch; ch += nw) {
    const int c = ch * 32 + cl;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
      const float* wp = p.weight + (size_t)c * 9 + tap;
      for (int s0 = 0; s0 < 16; s0 += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int s = s0 + u, n = 2 * s + half;
          const float wv = wp[(size_t)min(n, OMN - 1) * p.C * 9];
          bv[u] = n < OMN ? wv : 0.0f;
          av[u] = afrag[(tap * 16 + s) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);         // (all eight steps' loads ahead of their MFMAs)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (m < p.M) p.gx[(size_t)m * p.C + c] += acc[r];
    }
  }
}

int conv_bwd_check(const char* who, int B, int H, int W, int C) {
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  CF_REQUIRE(C > 0 && C % 32 == 0 && C <= 512, "%s: C=%d must be a multiple of 32, at most 512", who, C);
  const long M = (long)B * H * W;
  CF_REQUIRE(M * C < (1L << 31) && M * OMC < (1L << 31), "%s: tensor too large", who);
  return CF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// upsample backward.  Forward: out[yo, xo] += x[yi, xi] w[ky][kx] with yo = yi f - f / 2 + ky (ky < K = 2 f), likewise xo.
template <int K>
__global__ __launch_bounds__(256) void upsample_bwd_x_kernel(const float* __restrict__ gout, const float* __restrict__ w,
                                                             float* __restrict__ gx, int H, int W, int C4) {
  constexpr int F = K / 2, PAD = F / 2;
  const int yi = blockIdx.y, b = blockIdx.z;
  const int Ho = H * F, Wo = W * F;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(gout);
  const f32x4* w4 = reinterpret_cast<const f32x4*>(w);
  const int row_len = W * C4;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < row_len; j += gridDim.x * 256) {
    const int xi = j / C4, c4 = j - xi * C4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int yo = yi * F - PAD + ky;
      if (yo < 0 || yo >= Ho) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int xo = xi * F - PAD + kx;
        if (xo < 0 || xo >= Wo) continue;
        acc += g4[((size_t)(b * Ho + yo) * Wo + xo) * C4 + c4] * w4[(ky * K + kx) * C4 + c4];
      }
    }
    reinterpret_cast<f32x4*>(gx)[((size_t)(b * H + yi) * W) * C4 + j] = acc;
  }
}

// slab partials of gweight[ky][kx][c] = sum over the input pixels of x gout[yo, xo]: a workgroup = (slab of input pixels, ky)
template <int K>
__global__ __launch_bounds__(RED_T) void upsample_bwd_w_kernel(const float* __restrict__ gout, const float* __restrict__ x,
                                                               int H, int W, int C, long M, long slab_rows, float* __restrict__ ws) {
  constexpr int F = K / 2, PAD = F / 2;
  __shared__ f32x4 red[RED_T];
  const RowSplit s = row_split(C);
  const int ky = blockIdx.y;
  const int Ho = H * F, Wo = W * F;
  const long rb = (long)blockIdx.x * slab_rows, re = rb + slab_rows < M ? rb + slab_rows : M;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(gout);
  f32x4 acc[K];
#pragma unroll
  for (int kx = 0; kx < K; ++kx) acc[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s.active)
    for (long m = rb + s.rs; m < re; m += s.rpi) {
      const int b = (int)(m / ((long)H * W)), rem = (int)(m - (long)b * H * W);
      const int yi = rem / W, xi = rem - yi * W;
      const int yo = yi * F - PAD + ky;
      if (yo < 0 || yo >= Ho) continue;
      const f32x4 xv = reinterpret_cast<const f32x4*>(x)[m * s.C4 + s.c4];
      const f32x4* grow = g4 + ((size_t)(b * Ho + yo) * Wo) * s.C4 + s.c4;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int xo = xi * F - PAD + kx;
        if (xo >= 0 && xo < Wo) acc[kx] += xv * grow[(size_t)xo * s.C4];
      }
    }
  f32x4* w4 = reinterpret_cast<f32x4*>(ws + ((size_t)blockIdx.x * K + ky) * K * C);
#pragma unroll
  for (int kx = 0; kx < K; ++kx) {
    const f32x4 t = slot_sum(red, s, acc[kx]);
    if (threadIdx.x < (unsigned)s.C4) w4[kx * s.C4 + threadIdx.x] = t;
  }
}

// gweight[j] = sum over the slabs, in slab order, of ws[slab][j]
__global__ __launch_bounds__(256) void upsample_bwd_reduce_kernel(const float* __restrict__ ws, int slabs, int per,
                                                                  float* __restrict__ gweight) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= per) return;
  float v = ws[j];
  for (int z = 1; z < slabs; ++z) v += ws[(size_t)z * per + j];
  gweight[j] = v;
}

int up_check(const char* who, int B, int H, int W, int C, int f) {
  CF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024, "%s: bad geometry (C=%d: a multiple of 4, at most 1024)", who, C);
  CF_REQUIRE(f == 2 || f == 4, "%s: f=%d (2 or 4 only)", who, f);
  CF_REQUIRE(H < 65536 && B < 65536, "%s: too many rows / images for the launch grid", who);
  CF_REQUIRE((long)B * H * W * f * f * C < (1L << 40), "%s: tensor too large", who);
  return CF_OK;
}

}  // namespace

extern "C" int cf_offmask_activate(float* offmask, long M, void* stream) {
  CF_REQUIRE(offmask && M > 0 && M * OMC < (1L << 40), "cf_offmask_activate: bad arguments");
  CF_REQUIRE(reinterpret_cast<uintptr_t>(offmask) % 16 == 0, "cf_offmask_activate: the buffer must be 16-byte aligned");
  const long blocks = (M + 255) / 256;
  hipLaunchKernelGGL(offmask_activate_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, offmask, M);
  return cf_check_launch("cf_offmask_activate");
}

extern "C" size_t cf_conv3x3_bwd_workspace_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return 0;
  return (size_t)cw_slabs((long)B * H * W, C) * ((size_t)9 * OMN * C + OMN) * sizeof(float);
}

extern "C" int cf_conv3x3_bwd_weight(const float* gom, const float* offmask, const float* x, int B, int H, int W, int C,
                                     float* gw, float* gbias, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = conv_bwd_check("cf_conv3x3_bwd_weight", B, H, W, C)) return e;
  if (!gw && !gbias) return CF_OK;
  CF_REQUIRE(gom && offmask && (!gw || x), "cf_conv3x3_bwd_weight: null buffer");
  CF_REQUIRE(workspace && workspace_bytes >= cf_conv3x3_bwd_workspace_bytes(B, H, W, C),
             "cf_conv3x3_bwd_weight: workspace of %zu bytes is smaller than cf_conv3x3_bwd_workspace_bytes(...)", workspace_bytes);
  const long M = (long)B * H * W;
  const int slabs = cw_slabs(M, C);
  CwArgs k{};
  k.gom = gom; k.om = offmask; k.x = x ? x : gom; k.ws = static_cast<float*>(workspace);
  k.H = H; k.W = W; k.C = C; k.M = (int)M;
  k.slab_px = (int)((M + slabs - 1) / slabs);
  k.slab_px += k.slab_px & 1;                       // (two pixels per MFMA: slabs start on an even pixel)
  k.want_gw = gw != nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv3x3_bwd_weight_kernel, dim3((unsigned)slabs, k.want_gw ? (unsigned)(9 * (C / 32)) : 1u), dim3(64), 0, st, k);
  const long total = (gw ? 9L * OMN * C : 0) + (gbias ? OMN : 0);
  hipLaunchKernelGGL(conv3x3_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, k.ws, slabs, C, gw, gbias);
  return cf_check_launch("cf_conv3x3_bwd_weight");
}

extern "C" int cf_conv3x3_bwd_data(const float* gom, const float* offmask, const float* weight, int B, int H, int W, int C,
                                   float* gx, void* stream) {
  if (int e = conv_bwd_check("cf_conv3x3_bwd_data", B, H, W, C)) return e;
  CF_REQUIRE(gom && offmask && weight && gx, "cf_conv3x3_bwd_data: null buffer");
  CdArgs k{};
  k.gom = gom; k.om = offmask; k.weight = weight; k.gx = gx;
  k.H = H; k.W = W; k.C = C; k.M = B * H * W;
  const unsigned waves = (unsigned)(C / 32 < 4 ? C / 32 : 4);
  hipLaunchKernelGGL(conv3x3_bwd_data_kernel, dim3((unsigned)((k.M + CD_PX - 1) / CD_PX)), dim3(64 * waves), 0, (hipStream_t)stream, k);
  return cf_check_launch("cf_conv3x3_bwd_data");
}

extern "C" size_t cf_bn_relu_workspace_bytes(long M, int C) { return bn_workspace_bytes(M, C); }

extern "C" int cf_bn_relu_train_forward(const float* x, const float* gamma, const float* beta, float* running_mean,
                                        float* running_var, int training, float momentum, float eps, long M, int C, float* y,
                                        float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_train_forward("cf_bn_relu_train_forward", x, gamma, beta, nullptr, 1, running_mean, running_var, training, momentum, eps, M,
                          C, y, save_mean, save_invstd, workspace, workspace_bytes, stream);
}

extern "C" int cf_bn_relu_backward(const float* gy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                                   const float* save_invstd, int training, long M, int C, float* gz, float* ggamma, float* gbeta,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return bn_train_backward("cf_bn_relu_backward", gy, x, gamma, beta, nullptr, 1, save_mean, save_invstd, training, M, C, gz, nullptr,
                           ggamma, gbeta, workspace, workspace_bytes, stream);
}

extern "C" size_t cf_upsample_dw_bwd_workspace_bytes(int B, int H, int W, int C, int f) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || f <= 0) return 0;
  int slabs;
  long rows;
  red_slabs((long)B * H * W, &slabs, &rows);
  return (size_t)slabs * 4 * f * f * C * sizeof(float);
}

extern "C" int cf_upsample_dw_bwd(const float* gout, const float* x, const float* weight, int B, int H, int W, int C, int f,
                                  float* gx, float* gweight, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = up_check("cf_upsample_dw_bwd", B, H, W, C, f)) return e;
  if (!gx && !gweight) return CF_OK;
  CF_REQUIRE(gout && (!gx || weight) && (!gweight || x), "cf_upsample_dw_bwd: null buffer");
  CF_REQUIRE(aligned16({gout, x, weight, gx, gweight, workspace}), "cf_upsample_dw_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int C4 = C / 4;
  if (gx) {
    const dim3 grid((unsigned)((W * C4 + 255) / 256), (unsigned)H, (unsigned)B);
    if (f == 2) hipLaunchKernelGGL(upsample_bwd_x_kernel<4>, grid, dim3(256), 0, st, gout, weight, gx, H, W, C4);
    else hipLaunchKernelGGL(upsample_bwd_x_kernel<8>, grid, dim3(256), 0, st, gout, weight, gx, H, W, C4);
  }
  if (gweight) {
    CF_REQUIRE(workspace && workspace_bytes >= cf_upsample_dw_bwd_workspace_bytes(B, H, W, C, f),
               "cf_upsample_dw_bwd: workspace of %zu bytes is smaller than cf_upsample_dw_bwd_workspace_bytes(...)", workspace_bytes);
    const long M = (long)B * H * W;
    int slabs;
    long rows;
    red_slabs(M, &slabs, &rows);
    float* ws = static_cast<float*>(workspace);
    const int k = 2 * f, per = k * k * C;
    if (f == 2) hipLaunchKernelGGL(upsample_bwd_w_kernel<4>, dim3((unsigned)slabs, 4), dim3(RED_T), 0, st, gout, x, H, W, C, M, rows, ws);
    else hipLaunchKernelGGL(upsample_bwd_w_kernel<8>, dim3((unsigned)slabs, 8), dim3(RED_T), 0, st, gout, x, H, W, C, M, rows, ws);
    hipLaunchKernelGGL(upsample_bwd_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, ws, slabs, per, gweight);
  }
  return cf_check_launch("cf_upsample_dw_bwd");
}
