// DLA-34 stem for EARLY radar fusion in one launch (cf_stem.hip's kernel with a six-channel base layer): see the header comment
// of cf_stem.hip.  model/networks/fusionModules.py:18-35 (ConcateCombiner) + model/networks/dla.py:250-262.
#include "cf_stem_common.h"

namespace {

// Early fusion: P0 fills two patch planes, P1 runs 26 k-steps; the rest is the same text.
__global__ __launch_bounds__(256, 3) void stem_early_kernel(StemK p, StemRadar r) {
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

  // ---- P0, early fusion: the radar plane behind the image plane - the quarter-resolution map read at (y >> 2, x >> 2)
  //      (ConcateCombiner's nearest upsample, fusionModules.py:24-32), the image's pre-scale, zeros outside the image
  {
    constexpr int NQ = (ST_RI * ST_RI + 255) / 256;
    const long PHW = (long)r.ph * r.pw;
    f32x4v v[NQ];
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      const int q = tid + 256 * it;
      const int y = y_i + q / ST_RI, x = x_i + q % ST_RI;
      v[it] = f32x4v{0.f, 0.f, 0.f, 0.f};
      if (q < ST_RI * ST_RI && (interior || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W))) {
        const float* src = r.pc + (size_t)b * 3 * PHW + (size_t)(y >> 2) * r.pw + (x >> 2);
        v[it][0] = src[0];
        v[it][1] = src[PHW];
        v[it][2] = src[2 * PHW];
      }
    }
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
      const int q = tid + 256 * it;
      uint2 hi, lo;
      split4(v[it], hi, lo, p.a_img);
      if (q < ST_RI * ST_RI) *reinterpret_cast<u32x4*>(in_lds + ST_IN_B + q * 16) = u32x4{hi.x, hi.y, lo.x, lo.y};
    }
  }

  constexpr int NB = ST_RB * ST_RB;                          // 361
  constexpr int NTB = (NB + 15) / 16;                        // 23
  // ---- P1, early fusion: the same tiles (a wave owns tiles wave + 4 n, n = 0..5; tile 23 of wave 3 is a clamped spare), all six
  //      accumulators live, k-step-outer over the 13 image k-steps and then the 13 radar k-steps: per accumulator the image part is
  //      summed in cf_stem_fused's order, so zero radar weights give that kernel's bits
  constexpr int NT = 2 * ((NTB + 7) / 8);                    // 6
  const f32x4v bias_b = *reinterpret_cast<const f32x4v*>(p.b_base + 4 * kg);
  int q[NT];
  const unsigned char* src[NT];
  f32x4v acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    q[n] = min((wave + 4 * n) * 16 + col, NB - 1);
    src[n] = in_lds + ((q[n] / ST_RB) * ST_RI + q[n] % ST_RB) * 16;
    acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) {
    const unsigned char* w = pl ? r.w_radar : p.w_base;
#pragma unroll
    for (int ks = 0; ks < 13; ++ks) {
      const f16x8 w_hh = *sfrag(w, ks * 2 + 0, lane), w_l0 = *sfrag(w, ks * 2 + 1, lane);
      auto off = [](int tap) { tap = tap < 48 ? tap : 48; return ((tap / 7) * ST_RI + tap % 7) * 16; };
      const int o01 = kg & 1 ? off(4 * ks + 1) : off(4 * ks + 0), o23 = kg & 1 ? off(4 * ks + 3) : off(4 * ks + 2);
      const int toff = (kg & 2 ? o23 : o01) + pl * ST_IN_B;
      f16x8 xv[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) xv[n] = *reinterpret_cast<const f16x8*>(src[n] + toff);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_l0, xv[n], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_hh, xv[n], acc[n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int py = q[n] / ST_RB, px = q[n] - py * ST_RB;
    const int y = y_b + py, x = x_b + px;
    const bool inside = interior || ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W);
    f32x4v v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = inside ? fmaxf(acc[n][e] * p.s_base + bias_b[e], 0.0f) : 0.0f;
    uint2 hi, lo;
    split4(v, hi, lo, p.a_base);
    if ((wave + 4 * n) * 16 + col < NB) {
      *reinterpret_cast<uint2*>(base_lds + q[n] * ST_ROWB + 8 * kg) = hi;
      *reinterpret_cast<uint2*>(base_lds + q[n] * ST_ROWB + 32 + 8 * kg) = lo;
    }
  }

#include "cf_stem_tail.h"
}

}  // namespace

extern "C" int cf_stem_fused_early(const cf_stem_early_args* a, void* stream) {
  CF_REQUIRE(a != nullptr, "cf_stem_fused_early: null args");
  StemK k{};
  long blocks = 0;
  if (const int rc = stem_setup(&a->stem, "cf_stem_fused_early", k, blocks)) return rc;
  CF_REQUIRE(a->pc && a->w_base_radar, "cf_stem_fused_early: null radar map / radar weights");
  CF_REQUIRE(a->stem.H % 4 == 0 && a->stem.W % 4 == 0 && a->pc_h == a->stem.H / 4 && a->pc_w == a->stem.W / 4,
             "cf_stem_fused_early: the radar map must be exactly (H/4, W/4) with H, W multiples of 4 (H=%d W=%d, map %d x %d)",
             a->stem.H, a->stem.W, a->pc_h, a->pc_w);
  const StemRadar r{a->pc, a->pc_h, a->pc_w, reinterpret_cast<const unsigned char*>(a->w_base_radar)};
  static CfLdsLimit lds_limit;
  lds_limit.ensure(stem_early_kernel, ST_LDS, ST_LDS);
  hipLaunchKernelGGL(stem_early_kernel, dim3((unsigned)blocks), dim3(256), ST_LDS, (hipStream_t)stream, k, r);
  return cf_check_launch("cf_stem_fused_early");
}
