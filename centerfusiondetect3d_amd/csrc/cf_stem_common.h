// Shared by cf_stem.hip and cf_stem_early.hip: the stem kernels' geometry, kernel arguments and operand helpers, and the
// validation both entry points run.  (Two translation units: with both kernels in one, the three-channel kernel's
// instruction schedule changes - one unit per kernel keeps its code object what it was.)
#pragma once
#include "cf_f16x3.h"

namespace {


typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int ST_T1 = 8;                       // level1 tile edge
constexpr int ST_R0 = 2 * ST_T1 + 1;           // level0 region edge (17)
constexpr int ST_RB = ST_R0 + 2;               // base region edge (19)
constexpr int ST_RI = ST_RB + 6;               // image patch edge (25)
constexpr int ST_ROWB = 80;                    // bytes per region pixel: 16 ch hi (32) + lo (32) + pad
constexpr int ST_IN_B = ST_RI * ST_RI * 16;    // image patch: [px][4 hi | 4 lo]
constexpr int ST_BASE_B = ST_RB * ST_RB * ST_ROWB;
constexpr int ST_L0_B = ST_R0 * ST_R0 * ST_ROWB;
constexpr int ST_LDS = ST_BASE_B + ST_L0_B;    // 28,880 + 23,120 = 52,000 B: three workgroups per CU (the image
                                               // patch, dead once the base region exists, shares the level0 area)
static_assert(2 * ST_IN_B <= ST_L0_B, "the image patch and the radar patch (early fusion) must fit the level0 area");

struct StemK {
  const float* x;                 // NCHW fp32 (B, C, H, W), C <= 3 read
  int B, C, H, W;
  const unsigned char* w_base;    // [13 ks][2: {hi,hi} / {lo,0}][64 lanes][8 f16]
  const unsigned char* w_l0;      // [5 ks][2: hi / lo][64][8]
  const unsigned char* w_l1;      // [2 rt][5 ks][2][64][8]
  const float* b_base;            // 16
  const float* b_l0;              // 16
  const float* b_l1;              // 32
  float s_base, s_l0, s_l1;       // 2^-s / in_scale per layer
  float a_img, a_base, a_l0;      // activation pre-scales (in_scale): image, base_layer output, level0 output
  float* out;                     // fp32 NHWC (B, H/2, W/2, 32)
  float* out_pool;                // optional: its 2x2 / stride 2 max-pool, fp32 NHWC (B, H/4, W/4, 32)
  int tiles_x, tiles_y;
};

struct StemRadar {                // early fusion only
  const float* pc;                // NCHW fp32 (B, 3, ph, pw), ph = H / 4, pw = W / 4
  int ph, pw;
  const unsigned char* w_radar;   // [13 ks][2][64 lanes][8 f16]: w_base's layout for input channels 3..5, the same 2^s
};

__device__ __forceinline__ const f16x8* sfrag(const unsigned char* w, int idx, int lane) {
  return reinterpret_cast<const f16x8*>(w + ((size_t)idx * 64 + lane) * 16);
}

// 4 fp32 (one pixel, 4 consecutive channels) -> scaled, clamped fp16 hi / lo pairs
__device__ __forceinline__ void split4(const f32x4v& v, uint2& hi, uint2& lo, float in_scale) {
  const f32x4v xs = v * in_scale;
  split2(xs[0], xs[1], hi.x, lo.x);
  split2(xs[2], xs[3], hi.y, lo.y);
}

// validation and kernel arguments both entry points share; `who` names the entry point in the messages
[[maybe_unused]] static int stem_setup(const cf_stem_args* a, const char* who, StemK& k, long& blocks) {
  CF_REQUIRE(a->x && a->out, "%s: null tensor", who);
  CF_REQUIRE(a->B > 0 && a->C >= 1 && a->C <= 3, "%s: B=%d C=%d", who, a->B, a->C);
  CF_REQUIRE(a->H > 0 && a->W > 0 && a->H % 2 == 0 && a->W % 2 == 0, "%s: H=%d W=%d must be even", who, a->H, a->W);
  CF_REQUIRE(a->w_base && a->w_level0 && a->w_level1 && a->b_base && a->b_level0 && a->b_level1, "%s: null weights", who);
  CF_REQUIRE(a->scale_base > 0.f && a->scale_level0 > 0.f && a->scale_level1 > 0.f, "%s: out scales missing", who);
  k.x = a->x; k.B = a->B; k.C = a->C; k.H = a->H; k.W = a->W;
  k.w_base = reinterpret_cast<const unsigned char*>(a->w_base);
  k.w_l0 = reinterpret_cast<const unsigned char*>(a->w_level0);
  k.w_l1 = reinterpret_cast<const unsigned char*>(a->w_level1);
  k.b_base = a->b_base; k.b_l0 = a->b_level0; k.b_l1 = a->b_level1;
  k.s_base = a->scale_base; k.s_l0 = a->scale_level0; k.s_l1 = a->scale_level1;
  k.a_img = cf_resolve_in_scale(a->in_scale[0]); k.a_base = cf_resolve_in_scale(a->in_scale[1]); k.a_l0 = cf_resolve_in_scale(a->in_scale[2]);
  CF_REQUIRE(k.a_img > 0.f && k.a_base > 0.f && k.a_l0 > 0.f, "%s: in_scale must be 0 (= 16) or a power of two", who);
  k.out = a->out;
  k.out_pool = a->out_pool;
  k.tiles_x = (a->W / 2 + ST_T1 - 1) / ST_T1;
  k.tiles_y = (a->H / 2 + ST_T1 - 1) / ST_T1;
  blocks = (long)k.tiles_x * k.tiles_y * a->B;
  CF_REQUIRE(blocks < (1L << 31) && (long)a->B * a->C * a->H * a->W < (1L << 40), "%s: tensor too large", who);
  return CF_OK;
}


}  // namespace
