// Radar frustum association of the CenterFusion forward (and its replacement when MODEL.FRUSTUM is off): the secondary
// heads' pc_hm from the peaks of the primary heat map and the radar map.
//
// Integer / compare / scatter kernels bounded by HBM and LDS; the arithmetic that decides integer results (ROI bounds, gates,
// rounding) is written operation for operation like the reference's fp32 expressions, and this file is compiled with
// -ffp-contract=off so no multiply-add is fused behind our back.  The per-image radar map (3x112x200 = 269 KB) is
// L2-resident, and every ordering decision ("last painted box wins", "nearest radar point wins") is resolved inside LDS.
#include "cf_topk.h"

namespace {
constexpr int FR_THREADS = 1024;
constexpr int FR_SPLIT = 8;         // workgroups per image (pixel shares of the paint pass)
constexpr int FR_MAXK = 256;
constexpr int FR_NB = 4;          // boxes of a wave whose ROI loads are in flight together (8: slower - 37 vs 29 us on 40 x 30 boxes, 23 vs 21 on 9 x 7)
constexpr int PD_THREADS = 256;

struct FrBox {
  int roi_y0, roi_y1, roi_x0, roi_x1;  // ROI of pc_dep searched for a radar hit
  int p_y0, p_y1, p_x0, p_x1;          // rectangle painted on a hit
  float lo, hi;                        // strict depth gate
  float val[3];                        // painted values (depth/max_dist, vx, vz)
  int found;
};

// slice_keys != nullptr (cf_topk_frustum): the peaks arrive as the TOPK_SLICES sorted key lists of topk_slice_*_kernel and
// are merged HERE, by every workgroup of the image (3 us of redundant LDS work against a launch + 11 us); workgroup 0 of the
// image also writes them out as (scores, inds, classes) when asked.  Otherwise `inds` holds the K peaks (cf_frustum_assoc).
__global__ __launch_bounds__(FR_THREADS) void frustum_kernel(
    const int32_t* __restrict__ inds, int K, const float* __restrict__ depth, const float* __restrict__ wh,
    const float* __restrict__ dim, const float* __restrict__ rot, const float* __restrict__ calib,
    const float* __restrict__ pc_dep, int H, int W, float max_pc_dist, float* __restrict__ pc_hm,
    float* __restrict__ pc_hm_nhwc4, unsigned* __restrict__ pc_hm_split8, const uint64_t* __restrict__ slice_keys,
    float* __restrict__ tk_scores, int32_t* __restrict__ tk_inds, int32_t* __restrict__ tk_classes) {
  __shared__ FrBox box[FR_MAXK];
  __shared__ int s_pix[FR_MAXK];               // pixel of peak i
  __shared__ unsigned long long roi_best[FR_MAXK];   // ROI search: min over the gated returns of (value bits << 32 | position)
  __shared__ short cand[FR_MAXK];              // paint: the boxes that touch this workgroup's rows, last painted first
  __shared__ int s_ncand;
  extern __shared__ __attribute__((aligned(16))) uint64_t fr_keys[];   // slice_keys: topk_merge_lds_bytes(K)
  // FR_SPLIT workgroups per image: each rebuilds the (cheap) box table and paints its share of the
  // pixels - the per-pixel "last covering hit" scan is what takes the time
  const int b = blockIdx.x / FR_SPLIT, part = blockIdx.x % FR_SPLIT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  const float* dep_b = depth + (size_t)b * HW;
  const float* wh_b = wh + (size_t)b * 2 * HW;
  const float* dim_b = dim + (size_t)b * 3 * HW;
  const float* rot_b = rot + (size_t)b * 8 * HW;
  const float* cal = calib + (size_t)b * 12;
  const float* pc = pc_dep + (size_t)b * 3 * HW;

  if (slice_keys) {
    const int total = TOPK_SLICES * K;
    const uint64_t* src = slice_keys + (size_t)b * total;
    for (int i = tid; i < total; i += FR_THREADS) fr_keys[i] = src[i];
    __syncthreads();
    const uint64_t* best = merge_sorted_lists(fr_keys, fr_keys + total, K);
    if (tid < K) {
      float score;
      int pix, cls;
      unpack_key(best[tid], HW, score, pix, cls);
      s_pix[tid] = pix;
      if (part == 0 && tk_inds) {
        tk_scores[(size_t)b * K + tid] = score;
        tk_inds[(size_t)b * K + tid] = pix;
        tk_classes[(size_t)b * K + tid] = cls;
      }
    }
  } else if (tid < K) {
    s_pix[tid] = inds[(size_t)b * K + tid];
  }
  // (s_pix[tid] is read by the thread that wrote it)

  // ---- per-box geometry (utils/pointcloud.py:347-381, 397-437, 468-476)
  if (tid < K) {
    const int pix = s_pix[tid];
    const int yi = pix / W, xi = pix - yi * W;
    const float xs = (float)xi + 0.5f, ys = (float)yi + 0.5f;
    float w = wh_b[pix], h = wh_b[HW + pix];
    w = w < 0.0f ? 0.0f : w;
    h = h < 0.0f ? 0.0f : h;
    const float b0 = xs - w / 2.0f, b1 = ys - h / 2.0f, b2 = xs + w / 2.0f, b3 = ys + h / 2.0f;
    const float d = dep_b[pix];
    // get_alpha
    float r[8];
    for (int i = 0; i < 8; ++i) r[i] = rot_b[(size_t)i * HW + pix];
    const float idx = r[1] > r[5] ? 1.0f : 0.0f;
    const float a1 = atan2f(r[2], r[3]) + (float)(-0.5 * M_PI);
    const float a2 = atan2f(r[6], r[7]) + (float)(0.5 * M_PI);
    const float alpha = a1 * idx + a2 * (1.0f - idx);
    // getDistanceThresh: yaw, rotated box corners, max(z) - min(z)/2
    const float cx = (b0 + b2) / 2.0f, cy = (b1 + b3) / 2.0f;
    float yaw = alpha + atan2f(cx - cal[2], cal[0]);
    const float PI_F = (float)M_PI, TWO_PI_F = (float)(2.0 * M_PI);
    if (yaw > PI_F) yaw -= TWO_PI_F;
    if (yaw < -PI_F) yaw += TWO_PI_F;
    const float cs = cosf(yaw), sn = sinf(yaw);
    const float dh = dim_b[pix], dw = dim_b[HW + pix], dl = dim_b[2 * HW + pix];
    const float hx = 0.5f * dl, hz = 0.5f * dw;
    const float sx[4] = {hx, hx, -hx, -hx}, sz[4] = {hz, -hz, -hz, hz};
    float zmax = -INFINITY, zmin = INFINITY;
    for (int q = 0; q < 8; ++q) {
      const float yc = q < 4 ? 0.0f : -dh;
      const float z = ((-sn) * sx[q & 3] + 0.0f * yc) + cs * sz[q & 3];
      zmax = fmaxf(zmax, z);
      zmin = fminf(zmin, z);
    }
    const float thr = zmax - zmin / 2.0f;
    FrBox bx;
    py_slice((int)floorf(b1), (int)ceilf(b3) + 1, H, bx.roi_y0, bx.roi_y1);
    py_slice((int)floorf(b0), (int)ceilf(b2) + 1, W, bx.roi_x0, bx.roi_x1);
    bx.hi = d + thr;
    const float t = d - thr;
    bx.lo = t > 0.0f ? t : 0.0f;
    const float wi = 0.3f * (b2 - b0), hi_ = 0.3f * (b3 - b1);
    const int w_min = (int)(cx - wi / 2.0f), w_max = (int)(cx + wi / 2.0f);
    const int h_min = (int)(cy - hi_ / 2.0f), h_max = (int)(cy + hi_ / 2.0f);
    py_slice(h_min, h_max + 1, H, bx.p_y0, bx.p_y1);
    py_slice(w_min, w_max + 2, W, bx.p_x0, bx.p_x1);
    bx.found = 0;
    bx.val[0] = bx.val[1] = bx.val[2] = 0.0f;
    box[tid] = bx;
    roi_best[tid] = ~0ull;
  }
  __syncthreads();

  // ---- nearest gated radar return inside each ROI, row-major first-minimum.  A wave takes FR_NB of its boxes at a time (box
  //      i = g0 + 16 k) and walks their ROIs in rounds of 256 positions each: 4 FR_NB independent loads per lane and round.  The
  //      minimum is taken by ONE LDS atomic per lane and box on a 64-bit key (value bits << 32 | position): gated values are
  //      positive, so their bits order like the values, and among equal values the smallest position - the row-major first
  //      occurrence - wins.  No wave reduction (12 dependent cross-lane steps per box were 10 of this kernel's 32 us).
  constexpr int FR_WAVES = FR_THREADS / 64;
  for (int g0 = wave; g0 < K; g0 += FR_NB * FR_WAVES) {
    int rw[FR_NB], n[FR_NB], y0[FR_NB], x0[FR_NB];
    // magic = ceil(2^32 / rw) = (2^32 + e) / rw with e < rw: umulhi(q, magic) = floor(q / rw + q e / (2^32 rw)) == q / rw while
    // q e < 2^32.  A position is q < rw * H and rw <= W, so q e < W * W * H: below 2^32 by frustum_check.
    unsigned magic[FR_NB];
    float gl[FR_NB], gh[FR_NB];
    unsigned long long best[FR_NB];
    int n_max = 0;
#pragma unroll
    for (int k = 0; k < FR_NB; ++k) {
      const int i = g0 + k * FR_WAVES;
      const FrBox& bx = box[i < K ? i : g0];
      const int w_ = bx.roi_x1 - bx.roi_x0, h_ = bx.roi_y1 - bx.roi_y0;
      rw[k] = w_ > 1 ? w_ : 1;
      magic[k] = rw[k] > 1 ? (unsigned)((0x100000000ull + (unsigned)rw[k] - 1) / (unsigned)rw[k]) : 0u;
      n[k] = (i < K && w_ > 0 && h_ > 0) ? w_ * h_ : 0;
      y0[k] = bx.roi_y0; x0[k] = bx.roi_x0; gl[k] = bx.lo; gh[k] = bx.hi;
      best[k] = ~0ull;
      n_max = max(n_max, n[k]);
    }
    for (int base = 0; base < n_max; base += 256) {
      float v[FR_NB][4];
#pragma unroll
      for (int k = 0; k < FR_NB; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = base + lane + 64 * j;
          const int qq = q < n[k] ? q : 0;
          const int qr = rw[k] > 1 ? (int)__umulhi((unsigned)qq, magic[k]) : qq;       // qq / rw
          const float t = pc[(y0[k] + qr) * W + x0[k] + (qq - qr * rw[k])];          // (n[k] == 0: position 0 of a valid ROI origin or of box g0)
          v[k][j] = q < n[k] ? t : 0.0f;
        }
#pragma unroll
      for (int k = 0; k < FR_NB; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v[k][j] != 0.0f && v[k][j] < gh[k] && v[k][j] > gl[k]) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(v[k][j]) << 32) | (unsigned)(base + lane + 64 * j);
            best[k] = key < best[k] ? key : best[k];
          }
    }
#pragma unroll
    for (int k = 0; k < FR_NB; ++k)
      if (best[k] != ~0ull) atomicMin(&roi_best[g0 + k * FR_WAVES], best[k]);
  }
  __syncthreads();
  if (tid < K) {
    const unsigned long long key = roi_best[tid];
    if (key != ~0ull) {
      const FrBox& bx = box[tid];
      const int rw_ = bx.roi_x1 - bx.roi_x0, pos = (int)(unsigned)key;
      const int yy = bx.roi_y0 + pos / rw_, xx = bx.roi_x0 + pos % rw_;
      box[tid].found = 1;
      box[tid].val[0] = __uint_as_float((unsigned)(key >> 32)) / max_pc_dist;
      box[tid].val[1] = pc[HW + yy * W + xx];
      box[tid].val[2] = pc[2 * HW + yy * W + xx];
    }
  }
  __syncthreads();

  // ---- paint: boxes are drawn in top-k order, so for every pixel the LAST covering hit wins.  This workgroup paints
  //      pixels [p0, p_end): only the hits whose rectangle touches those rows are looked at, last painted first.
  float* hm = pc_hm + (size_t)b * 3 * HW;
  const int p_len = (HW + FR_SPLIT - 1) / FR_SPLIT;
  const int p0 = part * p_len, p_end = min(HW, (part + 1) * p_len);
  if (wave == 0) {
    const int y_lo = p0 / W, y_hi = p_end > p0 ? (p_end - 1) / W : y_lo;
    int n_c = 0;
    for (int base = 0; base < K; base += 64) {
      const int i = K - 1 - (base + lane);
      bool ok = false;
      if (i >= 0) {
        const FrBox& bx = box[i];
        ok = bx.found && bx.p_y0 <= y_hi && bx.p_y1 > y_lo && bx.p_x1 > bx.p_x0 && bx.p_y1 > bx.p_y0;
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) cand[n_c + __popcll(bal & ((1ull << lane) - 1ull))] = (short)i;
      n_c += (int)__popcll(bal);
    }
    if (lane == 0) s_ncand = n_c;
  }
  __syncthreads();
  const int n_cand = s_ncand;
  for (int p = p0 + tid; p < p_end; p += FR_THREADS) {
    const int y = p / W, x = p - y * W;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    for (int ci = 0; ci < n_cand; ++ci) {
      const FrBox& bx = box[cand[ci]];
      if (y >= bx.p_y0 && y < bx.p_y1 && x >= bx.p_x0 && x < bx.p_x1) {
        v0 = bx.val[0];
        v1 = bx.val[1];
        v2 = bx.val[2];
        break;
      }
    }
    hm[p] = v0;
    hm[HW + p] = v1;
    hm[2 * HW + p] = v2;
    if (pc_hm_nhwc4) {
      const f32x4 o = {v0, v1, v2, 0.0f};
      reinterpret_cast<f32x4*>(pc_hm_nhwc4)[(size_t)b * HW + p] = o;
    }
    if (pc_hm_split8) {  // [pixel][hi 8][lo 8] bf16, channels 3..7 zero
      const float h0 = (float)(__bf16)v0, h1 = (float)(__bf16)v1, h2 = (float)(__bf16)v2;
      auto pk = [](float a, float bq) {
        return ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)bq) << 16) |
               __builtin_bit_cast(unsigned short, (__bf16)a);
      };
      unsigned* o = pc_hm_split8 + ((size_t)b * HW + p) * 8;
      o[0] = pk(h0, h1); o[1] = pk(h2, 0.0f); o[2] = 0u; o[3] = 0u;
      o[4] = pk(v0 - h0, v1 - h1); o[5] = pk(v2 - h2, 0.0f); o[6] = 0u; o[7] = 0u;
    }
  }
}
}  // namespace

// What both entry points of frustum_kernel check (`buffers`: every pointer the caller needs is there).  The map bound comes
// first, so it can be seen without a buffer: the ROI search divides by multiplication (magic[] in the kernel), exact only
// while W * W * H < 2^32 - every map the model runs (200 * 200 * 112 = 4.5e6) is a thousandth of it.
static int frustum_check(const char* who, bool buffers, int K, int B, int H, int W) {
  // (in double: exact below 2^53, and no int W, H can overflow it)
  CF_REQUIRE((double)W * W * H < 4294967296.0, "%s: map of %d x %d: W * W * H must stay below 2^32 (the ROI search's division)", who, H, W);
  CF_REQUIRE(buffers, "%s: null buffer", who);
  CF_REQUIRE(K >= 1 && K <= FR_MAXK, "%s: K=%d outside [1,%d]", who, K, FR_MAXK);
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  return CF_OK;
}

extern "C" int cf_frustum_assoc(const int32_t* inds, int K, const float* depth, const float* wh,
                                const float* dim, const float* rot, const float* calib, const float* pc_dep,
                                int B, int H, int W, float max_pc_dist, float* pc_hm, float* pc_hm_nhwc4,
                                void* pc_hm_split8, void* stream) {
  if (const int e = frustum_check("cf_frustum_assoc", inds && depth && wh && dim && rot && calib && pc_dep && pc_hm, K, B, H, W))
    return e;
  hipLaunchKernelGGL(frustum_kernel, dim3(B * FR_SPLIT), dim3(FR_THREADS), 0, (hipStream_t)stream, inds, K, depth, wh, dim,
                     rot, calib, pc_dep, H, W, max_pc_dist, pc_hm, pc_hm_nhwc4, static_cast<unsigned*>(pc_hm_split8),
                     (const uint64_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  return cf_check_launch("cf_frustum_assoc");
}

// The chain between the two head launches in TWO launches instead of three: slice top-K of the raw heat map, then the
// frustum kernel, which merges the slices' lists in its prologue (the merge launch and its 11 us are gone).
extern "C" int cf_topk_frustum(const float* heat, int C, int K, const float* depth, const float* wh, const float* dim,
                               const float* rot, const float* calib, const float* pc_dep, int B, int H, int W,
                               float max_pc_dist, float* pc_hm, float* pc_hm_nhwc4, void* pc_hm_split8, float* scores,
                               int32_t* inds, int32_t* classes, void* workspace, void* stream) {
  if (const int e = frustum_check("cf_topk_frustum", heat && depth && wh && dim && rot && calib && pc_dep && pc_hm && workspace, K, B, H, W))
    return e;
  CF_REQUIRE((scores && inds && classes) || (!scores && !inds && !classes), "cf_topk_frustum: scores / inds / classes go together");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = topk_launch_slices("cf_topk_frustum", heat, B, C, H, W, K, 0, workspace, st)) return e;
  const size_t lds = topk_merge_lds_bytes(K);                      // <= 48 KB at K = 256, + 17 KB static
  static CfLdsLimit fr_limit;
  fr_limit.ensure(frustum_kernel, lds, 65536);
  hipLaunchKernelGGL(frustum_kernel, dim3(B * FR_SPLIT), dim3(FR_THREADS), lds, st, (const int32_t*)nullptr, K, depth, wh, dim,
                     rot, calib, pc_dep, H, W, max_pc_dist, pc_hm, pc_hm_nhwc4, static_cast<unsigned*>(pc_hm_split8),
                     static_cast<const uint64_t*>(workspace), scores, inds, classes);
  return cf_check_launch("cf_topk_frustum");
}

namespace {
// Middle fusion WITHOUT frustum association (base_model.py:69-79): the radar map itself is the secondary heads' pc_hm.
// One pass: channel 0 of pc_dep is normalised IN PLACE, x -> 1 - x / max_pc_dist (a true fp32 division, then the
// subtraction: the bits of torch's `x /= d; x = 1 - x` on the CPU), and the three channels are written channels-last in the
// two forms the secondary head launch reads - exactly what frustum_kernel writes.  V pixels per thread (V = 4: one
// 16-byte load per channel plane, 16-byte stores; V = 1 for maps / pointers that are not 16-byte aligned).
template <int V>
__global__ __launch_bounds__(PD_THREADS) void pc_hm_direct_kernel(float* __restrict__ pc_dep, long n_groups, int HW,
                                                                  float max_pc_dist, f32x4* __restrict__ pc_hm_nhwc4,
                                                                  u32x4p* __restrict__ pc_hm_split8) {
  const long g = (long)blockIdx.x * PD_THREADS + threadIdx.x;
  if (g >= n_groups) return;
  const long pix = g * V;                       // first pixel of the group, over B * HW (V divides HW: one image per group)
  const long b = pix / HW;
  float* p0 = pc_dep + b * 3 * (long)HW + (pix - b * HW);
  float v0[V], v1[V], v2[V];
  if constexpr (V == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p0);
    const f32x4 c = *reinterpret_cast<const f32x4*>(p0 + HW);
    const f32x4 d = *reinterpret_cast<const f32x4*>(p0 + 2 * (long)HW);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v0[i] = a[i]; v1[i] = c[i]; v2[i] = d[i]; }
  } else {
    v0[0] = p0[0]; v1[0] = p0[HW]; v2[0] = p0[2 * (long)HW];
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float q = v0[i] / max_pc_dist;
    v0[i] = 1.0f - q;
  }
  if constexpr (V == 4) {
    const f32x4 o = {v0[0], v0[1], v0[2], v0[3]};
    *reinterpret_cast<f32x4*>(p0) = o;
  } else {
    p0[0] = v0[0];
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    if (pc_hm_nhwc4) {
      const f32x4 o = {v0[i], v1[i], v2[i], 0.0f};
      pc_hm_nhwc4[pix + i] = o;
    }
    if (pc_hm_split8) {  // [pixel][hi 8][lo 8] bf16, channels 3..7 zero
      const float h0 = (float)(__bf16)v0[i], h1 = (float)(__bf16)v1[i], h2 = (float)(__bf16)v2[i];
      auto pk = [](float lo16, float hi16) {
        return ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)hi16) << 16) |
               __builtin_bit_cast(unsigned short, (__bf16)lo16);
      };
      const u32x4p hi = {pk(h0, h1), pk(h2, 0.0f), 0u, 0u};
      const u32x4p lo = {pk(v0[i] - h0, v1[i] - h1), pk(v2[i] - h2, 0.0f), 0u, 0u};
      pc_hm_split8[(pix + i) * 2] = hi;
      pc_hm_split8[(pix + i) * 2 + 1] = lo;
    }
  }
}
}  // namespace

extern "C" int cf_pc_hm_direct(float* pc_dep, int B, int H, int W, float max_pc_dist, float* pc_hm_nhwc4,
                               void* pc_hm_split8, void* stream) {
  CF_REQUIRE(pc_dep, "cf_pc_hm_direct: null pc_dep");
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "cf_pc_hm_direct: bad geometry (B=%d, H=%d, W=%d)", B, H, W);
  CF_REQUIRE((long)B * H * W < (1L << 31) / 3, "cf_pc_hm_direct: map of %ld pixels", (long)B * H * W);
  CF_REQUIRE(max_pc_dist > 0.0f, "cf_pc_hm_direct: max_pc_dist=%g must be positive", (double)max_pc_dist);
  CF_REQUIRE(((uintptr_t)pc_hm_nhwc4 & 15) == 0 && ((uintptr_t)pc_hm_split8 & 15) == 0,
             "cf_pc_hm_direct: pc_hm_nhwc4 / pc_hm_split8 must be 16-byte aligned");
  const int HW = H * W;
  const bool vec = (HW % 4 == 0) && (((uintptr_t)pc_dep & 15) == 0);
  const long n_groups = (long)B * HW / (vec ? 4 : 1);
  const unsigned blocks = (unsigned)((n_groups + PD_THREADS - 1) / PD_THREADS);
  hipLaunchKernelGGL(vec ? pc_hm_direct_kernel<4> : pc_hm_direct_kernel<1>, dim3(blocks), dim3(PD_THREADS), 0,
                     (hipStream_t)stream, pc_dep, n_groups, HW, max_pc_dist, reinterpret_cast<f32x4*>(pc_hm_nhwc4),
                     static_cast<u32x4p*>(pc_hm_split8));
  return cf_check_launch("cf_pc_hm_direct");
}
