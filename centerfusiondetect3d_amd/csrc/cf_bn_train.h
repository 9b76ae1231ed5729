// Training BatchNorm on an (M, C) fp32 map, shared by cf_neck_bwd.hip (cf_bn_relu_*: the DeformConv block) and cf_base_bwd.hip
// (cf_bn_act_*: the base's conv + BN blocks):  y = act(gamma (x - mean) invstd + beta [+ residual]),  act = ReLU or nothing.
// Batch statistics per slab of rows (two passes), the slabs merged in slab order in float64; every per-channel sum of the
// backward is a sum of slab partials added in slab order: bitwise reproducible, no float atomics.  With residual == NULL and
// relu == 1 every expression is the one cf_bn_relu_* has always evaluated.
#pragma once
#include "cf_common.h"
#include <initializer_list>

namespace {

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

// the forward's value in front of the activation: the affine, plus the residual where there is one
__device__ __forceinline__ f32x4 bn_pre_act(f32x4 v, const float* __restrict__ residual, long j) {
  return residual ? v + reinterpret_cast<const f32x4*>(residual)[j] : v;
}

__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ residual,
                                                            int relu, long total4, int C4, float* __restrict__ y) {
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  f32x4* y4 = reinterpret_cast<f32x4*>(y);
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total4; j += (long)gridDim.x * 256) {
    const int c4 = (int)(j % C4);
    f32x4 xh;
    const f32x4 v = bn_pre_act(bn_value(x4[j], reinterpret_cast<const f32x4*>(mean)[c4], reinterpret_cast<const f32x4*>(invstd)[c4],
                                        reinterpret_cast<const f32x4*>(gamma)[c4], reinterpret_cast<const f32x4*>(beta)[c4], &xh),
                               residual, j);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = relu ? fmaxf(v[e], 0.0f) : v[e];
    y4[j] = o;
  }
}

// slab partials of sum(g) and sum(g * xhat), g = gy where the activation passed
__global__ __launch_bounds__(RED_T) void bn_bwd_partial_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ residual, int relu, long M, int C,
                                                               long slab_rows, float* __restrict__ ws) {
  __shared__ f32x4 red[RED_T];
  const RowSplit s = row_split(C);
  const long rb = (long)blockIdx.x * slab_rows, re = rb + slab_rows < M ? rb + slab_rows : M;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s1 = zero, s2 = zero;
  if (s.active) {
    const f32x4 mu = reinterpret_cast<const f32x4*>(mean)[s.c4], is = reinterpret_cast<const f32x4*>(invstd)[s.c4];
    const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[s.c4], be = reinterpret_cast<const f32x4*>(beta)[s.c4];
    for (long r = rb + s.rs; r < re; r += s.rpi) {
      const long j = r * s.C4 + s.c4;
      const f32x4 g = reinterpret_cast<const f32x4*>(gy)[j];
      f32x4 xh;
      const f32x4 v = bn_pre_act(bn_value(reinterpret_cast<const f32x4*>(x)[j], mu, is, ga, be, &xh), residual, j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ge = (!relu || v[e] > 0.0f) ? g[e] : 0.0f;
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

// gz = gamma invstd (g - sum(g) / M - xhat sum(g xhat) / M); with the running statistics (sums == NULL) gamma invstd g.
// gres = g (the gradient of the residual: gy where the activation passed).  Either output may be NULL.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ residual, int relu,
                                                           const float* __restrict__ sums, float inv_m, long total4, int C4,
                                                           float* __restrict__ gz, float* __restrict__ gres) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total4; j += (long)gridDim.x * 256) {
    const int c4 = (int)(j % C4);
    const f32x4 is = reinterpret_cast<const f32x4*>(invstd)[c4], ga = reinterpret_cast<const f32x4*>(gamma)[c4];
    const f32x4 g = reinterpret_cast<const f32x4*>(gy)[j];
    f32x4 xh;
    const f32x4 v = bn_pre_act(bn_value(reinterpret_cast<const f32x4*>(x)[j], reinterpret_cast<const f32x4*>(mean)[c4], is, ga,
                                        reinterpret_cast<const f32x4*>(beta)[c4], &xh),
                               residual, j);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
    if (sums) {
      s1 = reinterpret_cast<const f32x4*>(sums)[c4];
      s2 = reinterpret_cast<const f32x4*>(sums)[C4 + c4];
    }
    f32x4 o, gm;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = (!relu || v[e] > 0.0f) ? g[e] : 0.0f;
      gm[e] = ge;
      o[e] = ga[e] * is[e] * (ge - s1[e] * inv_m - xh[e] * (s2[e] * inv_m));
    }
    if (gz) reinterpret_cast<f32x4*>(gz)[j] = o;
    if (gres) reinterpret_cast<f32x4*>(gres)[j] = gm;
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

size_t bn_workspace_bytes(long M, int C) {
  if (M <= 0 || C <= 0) return 0;
  int slabs;
  long rows;
  red_slabs(M, &slabs, &rows);
  return ((size_t)slabs * 3 + 2) * C * sizeof(float);
}

// the launches of cf_bn_relu_train_forward (residual = NULL, relu = 1) and cf_bn_act_train_forward; `who` names the entry point
int bn_train_forward(const char* who, const float* x, const float* gamma, const float* beta, const float* residual, int relu,
                     float* running_mean, float* running_var, int training, float momentum, float eps, long M, int C, float* y,
                     float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = bn_check(who, M, C)) return e;
  CF_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, "%s: null buffer", who);
  CF_REQUIRE(training || (running_mean && running_var), "%s: the running statistics are needed with training = 0", who);
  CF_REQUIRE(aligned16({x, gamma, beta, residual, y, save_mean, save_invstd, workspace}), "%s: buffers must be 16-byte aligned", who);
  CF_REQUIRE(!training || M > 1, "%s: batch statistics need more than one value per channel", who);
  hipStream_t st = (hipStream_t)stream;
  int slabs = 0;
  long rows = 0;
  if (training) {
    CF_REQUIRE(workspace && workspace_bytes >= bn_workspace_bytes(M, C),
               "%s: workspace of %zu bytes is smaller than its workspace_bytes function asks for", who, workspace_bytes);
    red_slabs(M, &slabs, &rows);
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)slabs), dim3(RED_T), 0, st, x, M, C, rows, static_cast<float*>(workspace));
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, static_cast<const float*>(workspace), slabs,
                     rows, M, C, training, momentum, eps, running_mean, running_var, save_mean, save_invstd);
  const long total4 = M * (C / 4);
  hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(stream_blocks(total4)), dim3(256), 0, st, x, gamma, beta, save_mean, save_invstd,
                     residual, relu, total4, C / 4, y);
  return cf_check_launch(who);
}

// the launches of cf_bn_relu_backward (residual = NULL, relu = 1, gres = NULL) and cf_bn_act_backward
int bn_train_backward(const char* who, const float* gy, const float* x, const float* gamma, const float* beta, const float* residual,
                      int relu, const float* save_mean, const float* save_invstd, int training, long M, int C, float* gz, float* gres,
                      float* ggamma, float* gbeta, void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = bn_check(who, M, C)) return e;
  if (!gz && !gres && !ggamma && !gbeta) return CF_OK;
  CF_REQUIRE(gy && x && gamma && beta && save_mean && save_invstd, "%s: null buffer", who);
  CF_REQUIRE(aligned16({gy, x, gamma, beta, residual, save_mean, save_invstd, gz, gres, workspace}),
             "%s: buffers must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  float* sums = nullptr;
  if ((training && gz) || ggamma || gbeta) {
    CF_REQUIRE(workspace && workspace_bytes >= bn_workspace_bytes(M, C),
               "%s: workspace of %zu bytes is smaller than its workspace_bytes function asks for", who, workspace_bytes);
    int slabs;
    long rows;
    red_slabs(M, &slabs, &rows);
    float* ws = static_cast<float*>(workspace);
    sums = ws + (size_t)slabs * 3 * C;
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)slabs), dim3(RED_T), 0, st, gy, x, gamma, beta, save_mean, save_invstd,
                       residual, relu, M, C, rows, ws);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, slabs, C, sums, ggamma, gbeta);
  }
  if (gz || gres) {
    const long total4 = M * (C / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(stream_blocks(total4)), dim3(256), 0, st, gy, x, gamma, beta, save_mean, save_invstd,
                       residual, relu, training ? sums : nullptr, 1.0f / (float)M, total4, C / 4, gz, gres);
  }
  return cf_check_launch(who);
}

}  // namespace
