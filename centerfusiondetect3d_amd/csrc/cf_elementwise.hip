// HBM-bound helpers of the DLA-34 / IDA-up graph: depthwise transposed-conv upsample (+ skip add),
// 2x2 max-pool, the layout changes at the module boundary and the fp32 -> split-bf16 conversion.
// All are one-pass streaming kernels: 16 B per lane, channel-innermost (NHWC) so every
// wave-instruction touches whole lines.
#include "cf_common.h"

namespace {

// out[b][y][x][c] = sum_{ky,kx} x[b][(y+p-ky)/f][(x+p-kx)/f][c] * w[ky][kx][c]  (+ skip)
// for the taps where (y+p-ky) and (x+p-kx) are multiples of f and in range; k = 2f, p = f/2, so
// exactly two ky (and two kx) qualify per output pixel.  Grid = (row segments, output rows, images):
// no per-element div / mod chain except the one split of the in-row index into (x, channel group);
// F is a template constant (2 or 4: shifts), 0 = any even f.
template <int F>
__global__ __launch_bounds__(256) void upsample_dw_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ skip,
                                                          float* __restrict__ out, int H, int W, int C4, int f_rt) {
  const int f = F ? F : f_rt;
  const int Ho = H * f, Wo = W * f, k = 2 * f, pad = f / 2;
  const int yo = blockIdx.y, b = blockIdx.z;
  const int ky0 = (yo + pad) % f;
  const int row_len = Wo * C4;
  const size_t row_base = ((size_t)b * Ho + yo) * row_len;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < row_len; j += gridDim.x * 256) {
    const int xo = j / C4, c4 = j - xo * C4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (skip) acc = reinterpret_cast<const f32x4*>(skip)[row_base + j];
    const int kx0 = (xo + pad) % f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int ky = ky0 + a * f;
      const int yi = (yo + pad - ky) / f;
      if (yi < 0 || yi >= H || ky >= k) continue;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const int kx = kx0 + bb * f;
        const int xi = (xo + pad - kx) / f;
        if (xi < 0 || xi >= W || kx >= k) continue;
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[((size_t)(b * H + yi) * W + xi) * C4 + c4];
        const f32x4 ww = reinterpret_cast<const f32x4*>(w)[(ky * k + kx) * C4 + c4];
        acc += v * ww;
      }
    }
    reinterpret_cast<f32x4*>(out)[row_base + j] = acc;
  }
}

// f = 2 (every upsample of the neck but one): a thread owns a 2 x 2 OUTPUT block of 4 channels.  The per-pixel kernel
// above issues 4 input + 4 weight + 1 skip load per output value group - each input row is requested 16 times and the
// vector-memory path, not HBM, sets its pace (207 MB in 50 us = 4.2 TB/s).  A block needs the 3 x 3 input neighbourhood
// once (9 loads for 16 taps) and the 16 weights once per THREAD (the in-row index advances by a multiple of C4, so a
// thread keeps its channel group): 17 memory instructions per 4 outputs instead of 40.  Every output is the same sum in
// the same order as upsample_dw_kernel<2> computes it (taps (ky0, kx0), (ky0, kx0 + 2), (ky0 + 2, kx0), (ky0 + 2, kx0 + 2);
// taps outside the input skipped): bit-identical.
__global__ __launch_bounds__(256) void upsample2_block_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ skip, float* __restrict__ out,
                                                              int H, int W, int C4) {
  const int i = blockIdx.y, b = blockIdx.z;          // input row
  const int Wo = 2 * W;
  const int row_len = W * C4;
  const int j0 = blockIdx.x * 256 + threadIdx.x;
  if (j0 >= row_len) return;
  const int c4 = j0 % C4;
  f32x4 ww[4][4];
#pragma unroll
  for (int ky = 0; ky < 4; ++ky)
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) ww[ky][kx] = reinterpret_cast<const f32x4*>(w)[(ky * 4 + kx) * C4 + c4];
  const bool up = i >= 1, dn = i + 1 < H;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x) + (size_t)(b * H + i) * W * C4;     // input row i
  const f32x4* xu = xr - (up ? (size_t)W * C4 : 0);                                       // row i - 1 (or a valid dummy)
  const f32x4* xd = xr + (dn ? (size_t)W * C4 : 0);                                       // row i + 1
  const size_t orow0 = ((size_t)b * 2 * H + 2 * i) * Wo * C4, orow1 = orow0 + (size_t)Wo * C4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int j = j0; j < row_len; j += gridDim.x * 256) {
    const int jx = j / C4;
    const bool lf = jx >= 1, rg = jx + 1 < W;
    const int cl = (lf ? jx - 1 : jx) * C4 + c4, cc = jx * C4 + c4, cr = (rg ? jx + 1 : jx) * C4 + c4;
    const f32x4 u0 = xu[cl], u1 = xu[cc], u2 = xu[cr];
    const f32x4 m0 = xr[cl], m1 = xr[cc], m2 = xr[cr];
    const f32x4 d0 = xd[cl], d1 = xd[cc], d2 = xd[cr];
    const size_t o00 = orow0 + (size_t)(2 * jx) * C4 + c4, o10 = orow1 + (size_t)(2 * jx) * C4 + c4;
    f32x4 a00 = zero, a01 = zero, a10 = zero, a11 = zero;
    if (skip) {
      a00 = reinterpret_cast<const f32x4*>(skip)[o00];
      a01 = reinterpret_cast<const f32x4*>(skip)[o00 + C4];
      a10 = reinterpret_cast<const f32x4*>(skip)[o10];
      a11 = reinterpret_cast<const f32x4*>(skip)[o10 + C4];
    }
    // output (2i, 2jx): ky in {1, 3} -> rows i, i - 1; kx in {1, 3} -> columns jx, jx - 1
    a00 += m1 * ww[1][1];
    if (lf) a00 += m0 * ww[1][3];
    if (up) a00 += u1 * ww[3][1];
    if (up && lf) a00 += u0 * ww[3][3];
    // output (2i, 2jx + 1): kx in {0, 2} -> columns jx + 1, jx
    if (rg) a01 += m2 * ww[1][0];
    a01 += m1 * ww[1][2];
    if (up && rg) a01 += u2 * ww[3][0];
    if (up) a01 += u1 * ww[3][2];
    // output (2i + 1, 2jx): ky in {0, 2} -> rows i + 1, i
    if (dn) a10 += d1 * ww[0][1];
    if (dn && lf) a10 += d0 * ww[0][3];
    a10 += m1 * ww[2][1];
    if (lf) a10 += m0 * ww[2][3];
    // output (2i + 1, 2jx + 1)
    if (dn && rg) a11 += d2 * ww[0][0];
    if (dn) a11 += d1 * ww[0][2];
    if (rg) a11 += m2 * ww[2][0];
    a11 += m1 * ww[2][2];
    reinterpret_cast<f32x4*>(out)[o00] = a00;
    reinterpret_cast<f32x4*>(out)[o00 + C4] = a01;
    reinterpret_cast<f32x4*>(out)[o10] = a10;
    reinterpret_cast<f32x4*>(out)[o10 + C4] = a11;
  }
}

// grid = (row segments, output rows, images): one split of the in-row index, no div / mod chain
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                         int H, int W, int C4) {
  const int Ho = H / 2, Wo = W / 2;
  const int yo = blockIdx.y, b = blockIdx.z;
  const int row_len = Wo * C4;
  const f32x4* in0 = reinterpret_cast<const f32x4*>(x) + ((size_t)(b * H + 2 * yo) * W) * C4;
  f32x4* o = reinterpret_cast<f32x4*>(out) + ((size_t)b * Ho + yo) * row_len;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < row_len; j += gridDim.x * 256) {
    const int xo = j / C4, c4 = j - xo * C4;
    const f32x4* p = in0 + (size_t)(2 * xo) * C4 + c4;
    const f32x4 a = p[0], bq = p[C4], c = p[(size_t)W * C4], d = p[(size_t)W * C4 + C4];
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaxf(fmaxf(a[e], bq[e]), fmaxf(c[e], d[e]));
    o[j] = r;
  }
}

__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                            int B, int C, long HW) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / HW, pix = i - b * HW;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) v[c] = x[(b * C + c) * HW + pix];
    reinterpret_cast<f32x4*>(out)[i] = v;
  }
}

// (B,H,W,c_stride) -> (B,C,H,W): 32-pixel x 32-channel tiles through LDS so both sides coalesce.
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           long HW, int C, int c_stride) {
  __shared__ float tile[32][33];
  const long p0 = (long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32, b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const long p = p0 + r;
    const int c = c0 + tx;
    tile[r][tx] = (p < HW && c < C) ? x[((long)b * HW + p) * c_stride + c] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const long p = p0 + tx;
    if (p < HW && c < C) out[((long)b * C + c) * HW + p] = tile[tx][r];
  }
}

// (B,C,H,W) -> (B,H,W,out_stride) at channel offset out_offset: the mirror image of nhwc_to_nchw_kernel (32 x 32 tiles
// through LDS, both sides coalesced).  Module-boundary helper of the operator-level deform_conv2d drop-in.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           long HW, int C, int out_stride, int out_offset) {
  __shared__ float tile[32][33];
  const long p0 = (long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32, b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const long p = p0 + tx;
    tile[r][tx] = (p < HW && c < C) ? x[((long)b * C + c) * HW + p] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long p = p0 + r;
    const int c = c0 + tx;
    if (p < HW && c < C) out[((long)b * HW + p) * out_stride + out_offset + c] = tile[tx][r];
  }
}

// One workgroup that keeps its CU slot busy for `ticks` of the 100 MHz constant clock (s_memrealtime): the probe
// host code uses to find out which HIP streams run concurrently (model.py: _side_streams).  Always terminates.
// max |x| over a strided fp32 matrix, as the BITS of the maximum (non-negative floats order like unsigned integers; a NaN's
// bits exceed +inf's, so a NaN anywhere comes out as NaN): wave shuffle reduction, one atomicMax per wave.
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long M, int C, int stride, unsigned* __restrict__ out) {
  unsigned best = 0u;
  const long step = (long)gridDim.x * 256;
  if (stride == C && (C & 3) == 0) {                       // contiguous rows: 16 bytes per lane
    const long n4 = M * C / 4;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
      const f32x4 v = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) best = max(best, __float_as_uint(v[e]) & 0x7fffffffu);
    }
  } else {
    const long n = M * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
      const long m = i / C;
      best = max(best, __float_as_uint(x[m * stride + (i - m * C)]) & 0x7fffffffu);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
  __shared__ unsigned part[4];                   // one atomic per block (same-address atomics are served one by one)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    best = max(max(part[0], part[1]), max(part[2], part[3]));
    if (best) atomicMax(out, best);
  }
}

__global__ __launch_bounds__(64) void spin_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ---- split-bf16: an fp32 value x carried as two bf16 numbers x = hi + lo (hi = rne(x), lo = rne(x - hi)): the operand format
// of the head kernels (cf_heads.hip).  A pixel is [Cs hi][Cs lo] bf16 - the same HBM bytes as fp32.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const __bf16 x = (__bf16)a, y = (__bf16)b;
  return ((unsigned)__builtin_bit_cast(unsigned short, y) << 16) | __builtin_bit_cast(unsigned short, x);
}
__device__ __forceinline__ float bf16_round(float a) { return (float)(__bf16)a; }

// fp32 NHWC [M][C] -> split-bf16 [M][2][Cs] (Cs >= C, channels C..Cs-1 zero), 8 channels per thread
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ x, unsigned char* __restrict__ out,
                                                         long M, int C, int in_stride, int Cs) {
  const int G = Cs / 8;
  const long total = M * G;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / G;
    const int c0 = (int)(i - m * G) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (c0 + e < C) ? x[m * in_stride + c0 + e] : 0.0f;
    u32x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bf16_round(v[2 * e]), b = bf16_round(v[2 * e + 1]);
      hi[e] = pack_bf16(a, b);
      lo[e] = pack_bf16(v[2 * e] - a, v[2 * e + 1] - b);
    }
    unsigned char* o = out + ((size_t)m * 2 * Cs + c0) * 2;
    *reinterpret_cast<u32x4*>(o) = hi;
    *reinterpret_cast<u32x4*>(o + (size_t)Cs * 2) = lo;
  }
}

inline int grid_for(long total) {
  long g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 256 * 16 ? 256 * 16 : g));
}

}  // namespace

extern "C" int cf_upsample_dw(const float* x, const float* weight, const float* skip, float* out, int B,
                              int H, int W, int C, int f, void* stream) {
  CF_REQUIRE(x && weight && out, "cf_upsample_dw: null buffer");
  CF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "cf_upsample_dw: bad geometry (C=%d)", C);
  CF_REQUIRE(f >= 2 && f % 2 == 0, "cf_upsample_dw: f=%d must be even (k=2f, pad=f/2)", f);
  CF_REQUIRE((long)H * f < 65536 && B < 65536, "cf_upsample_dw: too many rows / images for the launch grid");
  const int row_len = W * f * (C / 4);
  const dim3 grid((unsigned)((row_len + 255) / 256), (unsigned)(H * f), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  // f = 2 with a channel-group count that divides the workgroup: 2 x 2 output blocks per thread (same sums, same order);
  // other channel counts take the per-pixel kernel below.
  if (f == 2 && 256 % (C / 4) == 0) {
    const dim3 g2((unsigned)((W * (C / 4) + 255) / 256), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(upsample2_block_kernel, g2, dim3(256), 0, st, x, weight, skip, out, H, W, C / 4);
    return cf_check_launch("cf_upsample_dw");
  }
  if (f == 2)
    hipLaunchKernelGGL(upsample_dw_kernel<2>, grid, dim3(256), 0, st, x, weight, skip, out, H, W, C / 4, f);
  else if (f == 4)
    hipLaunchKernelGGL(upsample_dw_kernel<4>, grid, dim3(256), 0, st, x, weight, skip, out, H, W, C / 4, f);
  else
    hipLaunchKernelGGL(upsample_dw_kernel<0>, grid, dim3(256), 0, st, x, weight, skip, out, H, W, C / 4, f);
  return cf_check_launch("cf_upsample_dw");
}

extern "C" int cf_maxpool2x2(const float* x, float* out, int B, int H, int W, int C, void* stream) {
  CF_REQUIRE(x && out, "cf_maxpool2x2: null buffer");
  CF_REQUIRE(B > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "cf_maxpool2x2: bad geometry");
  CF_REQUIRE(H / 2 < 65536 && B < 65536, "cf_maxpool2x2: too many rows / images for the launch grid");
  const int row_len = (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((row_len + 255) / 256), (unsigned)(H / 2), (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, x, out, H, W, C / 4);
  return cf_check_launch("cf_maxpool2x2");
}

extern "C" int cf_nchw_to_nhwc4(const float* x, float* out, int B, int C, int H, int W, void* stream) {
  CF_REQUIRE(x && out, "cf_nchw_to_nhwc4: null buffer");
  CF_REQUIRE(B > 0 && C >= 1 && C <= 4 && H > 0 && W > 0, "cf_nchw_to_nhwc4: bad geometry (C=%d)", C);
  const long total = (long)B * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, B,
                     C, (long)H * W);
  return cf_check_launch("cf_nchw_to_nhwc4");
}

extern "C" int cf_nhwc_to_nchw(const float* x, float* out, int B, int H, int W, int C, int c_stride,
                               void* stream) {
  CF_REQUIRE(x && out, "cf_nhwc_to_nchw: null buffer");
  CF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && c_stride >= C, "cf_nhwc_to_nchw: bad geometry");
  const long HW = (long)H * W;
  dim3 grid((unsigned)((HW + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, out, HW, C, c_stride);
  return cf_check_launch("cf_nhwc_to_nchw");
}

extern "C" int cf_nchw_to_nhwc(const float* x, float* out, int B, int C, int H, int W, int out_stride, int out_offset,
                               void* stream) {
  CF_REQUIRE(x && out, "cf_nchw_to_nhwc: null buffer");
  CF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && out_offset >= 0 && out_stride >= out_offset + C,
             "cf_nchw_to_nhwc: bad geometry (C=%d, out_stride=%d, out_offset=%d)", C, out_stride, out_offset);
  const long HW = (long)H * W;
  CF_REQUIRE(B < 65536 && (C + 31) / 32 < 65536, "cf_nchw_to_nhwc: too many images / channels for the launch grid");
  dim3 grid((unsigned)((HW + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, out, HW, C, out_stride, out_offset);
  return cf_check_launch("cf_nchw_to_nhwc");
}

extern "C" int cf_absmax_f32(const float* x, long M, int C, int stride, float* out, void* stream) {
  CF_REQUIRE(x && out, "cf_absmax_f32: null buffer");
  CF_REQUIRE(M >= 0 && C > 0 && stride >= C, "cf_absmax_f32: bad geometry (M=%ld, C=%d, stride=%d)", M, C, stride);
  CF_REQUIRE(stride != C || (C & 3) != 0 || (reinterpret_cast<uintptr_t>(x) & 15) == 0, "cf_absmax_f32: contiguous rows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (const hipError_t e = hipMemsetAsync(out, 0, sizeof(float), st); e != hipSuccess) {
    cf_set_error("cf_absmax_f32: hipMemsetAsync failed: %s", hipGetErrorString(e));
    return CF_ELAUNCH;
  }
  if (M == 0) return CF_OK;
  const long n = M * C;
  const long blocks = (n / 4 + 255) / 256;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 512 ? 512 : blocks)), dim3(256), 0, st, x, M, C, stride,
                     reinterpret_cast<unsigned*>(out));
  return cf_check_launch("cf_absmax_f32");
}

extern "C" int cf_spin_us(int microseconds, void* stream) {
  CF_REQUIRE(microseconds > 0 && microseconds <= 100000, "cf_spin_us: %d us outside (0, 100000]", microseconds);
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)microseconds * 100ull);
  return cf_check_launch("cf_spin_us");
}

extern "C" int cf_split_bf16(const float* x, void* out, long M, int C, int in_stride, int Cs, void* stream) {
  CF_REQUIRE(x && out, "cf_split_bf16: null buffer");
  CF_REQUIRE(M > 0 && C > 0 && in_stride >= C && Cs >= C && Cs % 8 == 0, "cf_split_bf16: bad geometry");
  const long total = M * (Cs / 8);
  long g = (total + 255) / 256;
  if (g > 256 * 16) g = 256 * 16;
  hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x,
                     reinterpret_cast<unsigned char*>(out), M, C, in_stride, Cs);
  return cf_check_launch("cf_split_bf16");
}
