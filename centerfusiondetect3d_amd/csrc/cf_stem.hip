// DLA-34 stem in ONE launch:  images (NCHW, 3 ch)  ->  base_layer 7x7 (3 -> 16) + BN + ReLU
//                                                   ->  level0 3x3 (16 -> 16) + BN + ReLU
//                                                   ->  level1 3x3 stride 2 (16 -> 32) + BN + ReLU  (fp32 NHWC)
// (model/networks/dla.py:237-262: base_layer, level0, level1 of DLA.forward).  As separate launches
// these three layers move 1.7 GB of full-resolution activations through HBM for 66 GFLOP; fused, a
// workgroup keeps everything between the image and the half-resolution level1 map in LDS (52 KB):
//
//   level1 tile 8 x 8  <-  level0 region 17 x 17  <-  base region 19 x 19  <-  image patch 25 x 25
//
// Every region position outside the image is written as ZERO (each layer pads its OWN input with
// zeros - evaluating the previous layer outside the image would be wrong).
//
// Arithmetic: f16x3 as in cf_gemm_f16.hip (fp32 values split into fp16 hi + lo after a power-of-two
// scale, products on the f16 MFMA pipe, fp32 accumulation), here on v_mfma_f32_16x16x32_f16: 16 output
// channels are exactly one tile row, pixels are the columns (lane & 15), and a lane's 8 k-values
// (lane >> 4 selects the k group) are
//   * base_layer: ONE tap of the image patch, [4 ch hi | 4 ch lo] - a single 16-byte LDS read.  Both
//     halves meet the weights as  {w_hi, w_hi} . {x_hi, x_lo}  +  {w_lo, 0} . {x_hi, x_lo}, i.e. the same
//     three products  w_hi x_hi + w_hi x_lo + w_lo x_hi  in two MFMAs (13 k-steps of 4 taps; 49 taps + 3 pad);
//   * level0 / level1: 8 channels of one tap (k-step = 2 taps x 16 ch, 5 k-steps, tap 9 is padding),
//     hi and lo planes read separately, three MFMAs (main + two cross terms) as everywhere else.
// Weight fragments are packed on the host in exactly that lane order (packing.pack_stem).
//
// Early radar fusion (cf_stem_fused_early, cf_stem_early.hip; model/networks/fusionModules.py:18-35 + dla.py:250-262): the base
// layer has six input channels, [image | radar map nearest-upsampled x4].  That image is never built: a SECOND plane of the 25 x 25
// patch holds the radar values read at (y >> 2, x >> 2) of the quarter-resolution map, and the radar taps are 13 further k-steps
// into the same accumulators, behind the image's.  26 k-steps of fragments do not fit the registers at three workgroups per CU, so
// that kernel walks k-step-outer: a fragment pair is loaded once, meets all six tiles of the wave, and is gone
// (packing.pack_stem_early).  Levels 0 and 1 are the same text for both kernels: cf_stem_tail.h.
#include "cf_stem_common.h"

namespace {

__global__ __launch_bounds__(256, 3) void stem_kernel(StemK p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* base_lds = lds;
  unsigned char* l0_lds = lds + ST_BASE_B;
  unsigned char* in_lds = l0_lds;            // P0/P1 only; P2 starts behind a barrier

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kg = lane >> 4;
  const int per_img = p.tiles_x * p.tiles_y;
  const int b = blockIdx.x / per_img, rem = blockIdx.x - b * per_img;
  const int oy0 = (rem / p.tiles_x) * ST_T1, ox0 = (rem % p.tiles_x) * ST_T1;   // level1 tile origin
  const int y_l0 = 2 * oy0 - 1, x_l0 = 2 * ox0 - 1;          // level0 region origin (full resolution)
  const int y_b = y_l0 - 1, x_b = x_l0 - 1;                  // base region origin
  const int y_i = y_b - 3, x_i = x_b - 3;                    // image patch origin
  const long HW = (long)p.H * p.W;
  // workgroups whose whole image patch lies inside the image (almost all of them) skip every border test
  const bool interior = y_i >= 0 && x_i >= 0 && y_i + ST_RI <= p.H && x_i + ST_RI <= p.W;

  // ---- P0: image patch -> split fp16 -> LDS (zeros outside the image, channel 3 is zero); every load
  //      of the thread is in flight before the first one is used
  {
    constexpr int NQ = (ST_RI * ST_RI + 255) / 256;
    f32x4v v[NQ];
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      const int q = tid + 256 * it;
      const int y = y_i + q / ST_RI, x = x_i + q % ST_RI;
      v[it] = f32x4v{0.f, 0.f, 0.f, 0.f};
      if (q < ST_RI * ST_RI && (interior || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W))) {
        const float* src = p.x + (size_t)b * p.C * HW + (size_t)y * p.W + x;
        v[it][0] = src[0];
        if (p.C > 1) v[it][1] = src[HW];
        if (p.C > 2) v[it][2] = src[2 * HW];
      }
    }
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      const int q = tid + 256 * it;
      uint2 hi, lo;
      split4(v[it], hi, lo, p.a_img);
      if (q < ST_RI * ST_RI) *reinterpret_cast<u32x4*>(in_lds + q * 16) = u32x4{hi.x, hi.y, lo.x, lo.y};
    }
  }

  // ---- P1 weights (both variants of all 13 k-steps stay in registers) and per-lane tap offsets
  f16x8 wb[13][2];
  int toff[13];
#pragma unroll
  for (int ks = 0; ks < 13; ++ks) {
    wb[ks][0] = *sfrag(p.w_base, ks * 2 + 0, lane);
    wb[ks][1] = *sfrag(p.w_base, ks * 2 + 1, lane);
    // taps 49..51 are padding (zero weights).  Four compile-time candidates, one select per k group:
    // no per-lane division chain
    auto off = [](int tap) { tap = tap < 48 ? tap : 48; return ((tap / 7) * ST_RI + tap % 7) * 16; };
    const int o01 = kg & 1 ? off(4 * ks + 1) : off(4 * ks + 0), o23 = kg & 1 ? off(4 * ks + 3) : off(4 * ks + 2);
    toff[ks] = kg & 2 ? o23 : o01;
  }
  const f32x4v bias_b = *reinterpret_cast<const f32x4v*>(p.b_base + 4 * kg);
  __syncthreads();

  // ---- P1: base_layer over the 19 x 19 region, 16 pixels per MFMA tile, two tiles in flight per wave
  //      (independent accumulators keep the MFMA pipe busy between dependent steps)
  constexpr int NB = ST_RB * ST_RB;                          // 361
  constexpr int NTB = (NB + 15) / 16;                        // 23
  for (int t0 = wave; t0 < NTB; t0 += 8) {
    int q[2], py[2], px[2];
    const unsigned char* src[2];
    f32x4v acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      q[u] = min((t0 + 4 * u) * 16 + col, NB - 1);
      py[u] = q[u] / ST_RB;
      px[u] = q[u] - py[u] * ST_RB;
      src[u] = in_lds + (py[u] * ST_RI + px[u]) * 16;
      acc[u] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < 13; ++ks) {
      f16x8 xv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) xv[u] = *reinterpret_cast<const f16x8*>(src[u] + toff[ks]);
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ks][1], xv[u], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ks][0], xv[u], acc[u], 0, 0, 0);
    }
    // lane = (pixel col, channel group kg): channels 4kg..4kg+3 of pixel q
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int y = y_b + py[u], x = x_b + px[u];
      const bool inside = interior || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W);
      f32x4v v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = inside ? fmaxf(acc[u][e] * p.s_base + bias_b[e], 0.0f) : 0.0f;
      uint2 hi, lo;
      split4(v, hi, lo, p.a_base);
      if ((t0 + 4 * u) * 16 + col < NB) {
        *reinterpret_cast<uint2*>(base_lds + q[u] * ST_ROWB + 8 * kg) = hi;
        *reinterpret_cast<uint2*>(base_lds + q[u] * ST_ROWB + 32 + 8 * kg) = lo;
      }
    }
  }

#include "cf_stem_tail.h"
}

}  // namespace

extern "C" int cf_stem_fused(const cf_stem_args* a, void* stream) {
  CF_REQUIRE(a != nullptr, "cf_stem_fused: null args");
  StemK k{};
  long blocks = 0;
  if (const int rc = stem_setup(a, "cf_stem_fused", k, blocks)) return rc;
  static CfLdsLimit lds_limit;
  lds_limit.ensure(stem_kernel, ST_LDS, ST_LDS);
  hipLaunchKernelGGL(stem_kernel, dim3((unsigned)blocks), dim3(256), ST_LDS, (hipStream_t)stream, k);
  return cf_check_launch("cf_stem_fused");
}

