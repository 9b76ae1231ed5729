// Training kernels of the neck's DeformConv block and IDA upsample (ops.deform_conv_block / ops.upsample_dw_add), fp32 NHWC:
//
//   cf_offmask_activate       sigmoid of the mask logits in the offset convolution's output, in place
//   cf_conv3x3_bwd_weight     gw (27,C,3,3) / gbias (27) of conv_offset_mask from the DCN backward's gom and the block input
//   cf_conv3x3_bwd_data       gx += conv_offset_mask's input gradient (plain read-modify-write behind the DCN's atomics)
//   cf_bn_relu_train_forward  batch statistics (slab-local two-pass, slabs merged in float64), running statistics, y = relu(bn(x))
//   cf_bn_relu_backward       gz, ggamma, gbeta from gy and the saved pre-BN map
//   cf_upsample_dw_bwd        gx / gweight of cf_upsample_dw
//
// The two convolution kernels read gom with the mask derivative folded in on load: channels 18..26 of gom are the gradient with
// respect to the ACTIVATED mask m (saved in offmask), the convolution produced its logit, so they are multiplied by m (1 - m).
// Products that go through MFMA use the exact fp32-input v_mfma_f32_32x32x2_f32.  Every parameter gradient is a sum of slab
// partials added in slab order by a second launch: bitwise reproducible, no float atomics anywhere in this file.
#include "cf_common.h"
#include <initializer_list>

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
// Column reductions of an (M, C) map, shared by the batch-norm and upsample kernels: a workgroup of 256 threads holds
// 256 / (C / 4) rows of 16-byte channel groups; the rows' partials meet in LDS and are added in row-slot order.
constexpr int RED_T = 256;

struct RowSplit {
  int C4, rpi, rs, c4;
  bool active;
};

__device__ __forceinline__ RowSplit row_split(int C) {
  RowSplit s;
  s.C4 = C >> 2;
  s.rpi = RED_T / s.C4;
  s.rs = threadIdx.x / s.C4;
  s.c4 = threadIdx.x - s.rs * s.C4;
  s.active = s.rs < s.rpi;
  return s;
}

// sum over the row slots, in slot order: valid in the threads with tid < C4 (their channel group is tid)
__device__ __forceinline__ f32x4 slot_sum(f32x4* red, const RowSplit& s, f32x4 v) {
  __syncthreads();
  red[threadIdx.x] = s.active ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  f32x4 t = red[threadIdx.x < (unsigned)s.C4 ? threadIdx.x : 0];
  if (threadIdx.x < (unsigned)s.C4)
    for (int k = 1; k < s.rpi; ++k) t += red[k * s.C4 + threadIdx.x];
  return t;
}

// row slabs of the column reductions: about 128 rows each, 256 slabs at the most (the second launch walks them in order)
void red_slabs(long M, int* slabs, long* slab_rows) {
  long s0 = (M + 127) / 128;
  if (s0 > 256) s0 = 256;
  if (s0 < 1) s0 = 1;
  *slab_rows = (M + s0 - 1) / s0;
  *slabs = (int)((M + *slab_rows - 1) / *slab_rows);
}

__device__ __forceinline__ f32x4 bn_value(f32x4 x, f32x4 mean, f32x4 invstd, f32x4 gamma, f32x4 beta, f32x4* xh) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    (*xh)[e] = (x[e] - mean[e]) * invstd[e];
    v[e] = fmaf((*xh)[e], gamma[e], beta[e]);
  }
  return v;
}

// Slab statistics, two passes over the slab (the second one finds it in cache): the mean as pivot + mean of (x - pivot), the
// pivot being the slab's first row (so a large common offset cancels exactly), then the sum of squares about that mean.
__global__ __launch_bounds__(RED_T) void bn_stats_kernel(const float* __restrict__ x, long M, int C, long slab_rows,
                                                         float* __restrict__ ws) {
  __shared__ f32x4 red[RED_T];
  __shared__ f32x4 smean[RED_T];
  const RowSplit s = row_split(C);
  const long rb = (long)blockIdx.x * slab_rows, re = rb + slab_rows < M ? rb + slab_rows : M;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 piv = s.active ? x4[rb * s.C4 + s.c4] : zero;
  f32x4 a = zero;
  if (s.active)
    for (long r = rb + s.rs; r < re; r += s.rpi) a += x4[r * s.C4 + s.c4] - piv;
  f32x4 t = slot_sum(red, s, a);
  const float inv_n = 1.0f / (float)(re - rb);
  if (threadIdx.x < (unsigned)s.C4) {
    t *= inv_n;
    smean[threadIdx.x] = t;
  }
  __syncthreads();
  const f32x4 d = s.active ? smean[s.c4] : zero;
  const f32x4 mu = piv + d;
  f32x4 q = zero;
  if (s.active)
    for (long r = rb + s.rs; r < re; r += s.rpi) {
      const f32x4 e = x4[r * s.C4 + s.c4] - mu;
      q += e * e;
    }
  const f32x4 m2 = slot_sum(red, s, q);
  if (threadIdx.x < (unsigned)s.C4) {
    f32x4* w4 = reinterpret_cast<f32x4*>(ws + (size_t)blockIdx.x * 3 * C);
    w4[threadIdx.x] = piv;                // (row slot 0: the slab's first row)
    w4[s.C4 + threadIdx.x] = d;
    w4[2 * s.C4 + threadIdx.x] = m2;
  }
}

// One thread per channel: the slabs merged in slab order (Chan's update, in float64), then mean / invstd, and the running
// statistics (momentum; the unbiased variance).  training = 0: mean / invstd of the running statistics, nothing else.
__global__ __launch_bounds__(64) void bn_finalize_kernel(const float* __restrict__ ws, int slabs, long slab_rows, long M, int C,
                                                         int training, float momentum, float eps, float* __restrict__ running_mean,
                                                         float* __restrict__ running_var, float* __restrict__ save_mean,
                                                         float* __restrict__ save_invstd) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  if (!training) {
    save_mean[c] = running_mean[c];
    save_invstd[c] = 1.0f / sqrtf(running_var[c] + eps);
    return;
  }
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int z = 0; z < slabs; ++z) {
    const float* w = ws + (size_t)z * 3 * C;
    const long rb = (long)z * slab_rows;
    const double nb = (double)((rb + slab_rows < M ? rb + slab_rows : M) - rb);
    const double mb = (double)w[c] + (double)w[C + c];
    const double delta = mb - mean, nn = n + nb;
    mean += delta * (nb / nn);
    m2 += (double)w[2 * C + c] + delta * delta * (n * nb / nn);
    n = nn;
  }
  const float var = (float)(m2 / (double)M);
  save_mean[c] = (float)mean;
  save_invstd[c] = 1.0f / sqrtf(var + eps);
  if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
  if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(m2 / (double)(M - 1));
}

__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, long total4, int C4,
                                                            float* __restrict__ y) {
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  f32x4* y4 = reinterpret_cast<f32x4*>(y);
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total4; j += (long)gridDim.x * 256) {
    const int c4 = (int)(j % C4);
    f32x4 xh;
    const f32x4 v = bn_value(x4[j], reinterpret_cast<const f32x4*>(mean)[c4], reinterpret_cast<const f32x4*>(invstd)[c4],
                             reinterpret_cast<const f32x4*>(gamma)[c4], reinterpret_cast<const f32x4*>(beta)[c4], &xh);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(v[e], 0.0f);
    y4[j] = o;
  }
}

// slab partials of sum(g) and sum(g * xhat), g = gy where the ReLU passed
__global__ __launch_bounds__(RED_T) void bn_bwd_partial_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               long M, int C, long slab_rows, float* __restrict__ ws) {
  __shared__ f32x4 red[RED_T];
  const RowSplit s = row_split(C);
  const long rb = (long)blockIdx.x * slab_rows, re = rb + slab_rows < M ? rb + slab_rows : M;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s1 = zero, s2 = zero;
  if (s.active) {
    const f32x4 mu = reinterpret_cast<const f32x4*>(mean)[s.c4], is = reinterpret_cast<const f32x4*>(invstd)[s.c4];
    const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[s.c4], be = reinterpret_cast<const f32x4*>(beta)[s.c4];
    for (long r = rb + s.rs; r < re; r += s.rpi) {
      const f32x4 g = reinterpret_cast<const f32x4*>(gy)[r * s.C4 + s.c4];
      f32x4 xh;
      const f32x4 v = bn_value(reinterpret_cast<const f32x4*>(x)[r * s.C4 + s.c4], mu, is, ga, be, &xh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ge = v[e] > 0.0f ? g[e] : 0.0f;
        s1[e] += ge;
        s2[e] = fmaf(ge, xh[e], s2[e]);
      }
    }
  }
  const f32x4 t1 = slot_sum(red, s, s1);
  const f32x4 t2 = slot_sum(red, s, s2);
  if (threadIdx.x < (unsigned)s.C4) {
    f32x4* w4 = reinterpret_cast<f32x4*>(ws + (size_t)blockIdx.x * 2 * C);
    w4[threadIdx.x] = t1;
    w4[s.C4 + threadIdx.x] = t2;
  }
}

// the slab partials added in slab order (float64, rounded once): sums[0][C] = gbeta, sums[1][C] = ggamma
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(const float* __restrict__ ws, int slabs, int C, float* __restrict__ sums,
                                                             float* __restrict__ ggamma, float* __restrict__ gbeta) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int z = 0; z < slabs; ++z) {
    a += (double)ws[(size_t)z * 2 * C + c];
    b += (double)ws[(size_t)z * 2 * C + C + c];
  }
  sums[c] = (float)a;
  sums[C + c] = (float)b;
  if (gbeta) gbeta[c] = (float)a;
  if (ggamma) ggamma[c] = (float)b;
}

// gz = gamma invstd (g - sum(g) / M - xhat sum(g xhat) / M); with the running statistics (sums == NULL) gamma invstd g
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ sums, float inv_m, long total4, int C4,
                                                           float* __restrict__ gz) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total4; j += (long)gridDim.x * 256) {
    const int c4 = (int)(j % C4);
    const f32x4 is = reinterpret_cast<const f32x4*>(invstd)[c4], ga = reinterpret_cast<const f32x4*>(gamma)[c4];
    const f32x4 g = reinterpret_cast<const f32x4*>(gy)[j];
    f32x4 xh;
    const f32x4 v = bn_value(reinterpret_cast<const f32x4*>(x)[j], reinterpret_cast<const f32x4*>(mean)[c4], is, ga,
                             reinterpret_cast<const f32x4*>(beta)[c4], &xh);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
    if (sums) {
      s1 = reinterpret_cast<const f32x4*>(sums)[c4];
      s2 = reinterpret_cast<const f32x4*>(sums)[C4 + c4];
    }
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = v[e] > 0.0f ? g[e] : 0.0f;
      o[e] = ga[e] * is[e] * (ge - s1[e] * inv_m - xh[e] * (s2[e] * inv_m));
    }
    reinterpret_cast<f32x4*>(gz)[j] = o;
  }
}

int bn_check(const char* who, long M, int C) {
  CF_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && C <= 1024, "%s: bad geometry (M=%ld, C=%d: a multiple of 4, at most 1024)", who, M, C);
  CF_REQUIRE(M * C < (1L << 40), "%s: tensor too large", who);
  return CF_OK;
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* q : ps)
    if (reinterpret_cast<uintptr_t>(q) % 16) return false;
  return true;
}

unsigned stream_blocks(long total4) {
  const long b = (total4 + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b < 8192 ? b : 8192);
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

extern "C" size_t cf_bn_relu_workspace_bytes(long M, int C) {
  if (M <= 0 || C <= 0) return 0;
  int slabs;
  long rows;
  red_slabs(M, &slabs, &rows);
  return ((size_t)slabs * 3 + 2) * C * sizeof(float);
}

extern "C" int cf_bn_relu_train_forward(const float* x, const float* gamma, const float* beta, float* running_mean,
                                        float* running_var, int training, float momentum, float eps, long M, int C, float* y,
                                        float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = bn_check("cf_bn_relu_train_forward", M, C)) return e;
  CF_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, "cf_bn_relu_train_forward: null buffer");
  CF_REQUIRE(training || (running_mean && running_var), "cf_bn_relu_train_forward: the running statistics are needed with training = 0");
  CF_REQUIRE(aligned16({x, gamma, beta, y, save_mean, save_invstd, workspace}), "cf_bn_relu_train_forward: buffers must be 16-byte aligned");
  CF_REQUIRE(!training || M > 1, "cf_bn_relu_train_forward: batch statistics need more than one value per channel");
  hipStream_t st = (hipStream_t)stream;
  int slabs = 0;
  long rows = 0;
  if (training) {
    CF_REQUIRE(workspace && workspace_bytes >= cf_bn_relu_workspace_bytes(M, C),
               "cf_bn_relu_train_forward: workspace of %zu bytes is smaller than cf_bn_relu_workspace_bytes(...)", workspace_bytes);
    red_slabs(M, &slabs, &rows);
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)slabs), dim3(RED_T), 0, st, x, M, C, rows, static_cast<float*>(workspace));
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, static_cast<const float*>(workspace), slabs,
                     rows, M, C, training, momentum, eps, running_mean, running_var, save_mean, save_invstd);
  const long total4 = M * (C / 4);
  hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(stream_blocks(total4)), dim3(256), 0, st, x, gamma, beta, save_mean, save_invstd,
                     total4, C / 4, y);
  return cf_check_launch("cf_bn_relu_train_forward");
}

extern "C" int cf_bn_relu_backward(const float* gy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                                   const float* save_invstd, int training, long M, int C, float* gz, float* ggamma, float* gbeta,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = bn_check("cf_bn_relu_backward", M, C)) return e;
  if (!gz && !ggamma && !gbeta) return CF_OK;
  CF_REQUIRE(gy && x && gamma && beta && save_mean && save_invstd, "cf_bn_relu_backward: null buffer");
  CF_REQUIRE(aligned16({gy, x, gamma, beta, save_mean, save_invstd, gz, workspace}), "cf_bn_relu_backward: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* sums = nullptr;
  if (training || ggamma || gbeta) {
    CF_REQUIRE(workspace && workspace_bytes >= cf_bn_relu_workspace_bytes(M, C),
               "cf_bn_relu_backward: workspace of %zu bytes is smaller than cf_bn_relu_workspace_bytes(...)", workspace_bytes);
    int slabs;
    long rows;
    red_slabs(M, &slabs, &rows);
    float* ws = static_cast<float*>(workspace);
    sums = ws + (size_t)slabs * 3 * C;
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)slabs), dim3(RED_T), 0, st, gy, x, gamma, beta, save_mean, save_invstd, M,
                       C, rows, ws);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, slabs, C, sums, ggamma, gbeta);
  }
  if (gz) {
    const long total4 = M * (C / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(stream_blocks(total4)), dim3(256), 0, st, gy, x, gamma, beta, save_mean, save_invstd,
                       training ? sums : nullptr, 1.0f / (float)M, total4, C / 4, gz);
  }
  return cf_check_launch("cf_bn_relu_backward");
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
