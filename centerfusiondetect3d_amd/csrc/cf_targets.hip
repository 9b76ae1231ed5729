// Training targets on the device (cf_targets_build, include/cf_hip.h): the per-object host loops of the reference's dataset -
// dataset/generic_dataset.py:206-239 (the loop over annotations), 441-687 (initReturn, transformBbox, addInstance),
// dataset/datasets/nuscenes.py:348-391 (initReturn), utils/image.py:145-256 (getGaussianRadius, drawGaussianHeatRegion) and
// utils/pointcloud.py:214-328, 397-481 (cvtAlphaToYaw, get3DCorners, getDistanceThresh, cvtPcDepthToHeatmap on numpy inputs) -
// as three launches: one thread per (image, annotation), then the heat map and the ground-truth frustum map per (image, row band).
// Built with -ffp-contract=off: every decision (clip, truncation, gate) and every rounding follows numpy's dtypes operation by
// operation - float64 where numpy promotes, fp32 where it stores (NEP 50 rules: a Python scalar takes the array's or the numpy
// scalar's type).
#include "cf_common.h"
#include <math.h>

namespace {

constexpr int TGT_THREADS = 256;
constexpr int TGT_BAND = 16;        // map rows per workgroup of the two map kernels
constexpr double TGT_PI = 3.141592653589793;

// what the object kernel leaves for the two map kernels (one per (image, annotation); valid = 0 for a skipped row)
struct TgtDesc {
  int32_t valid, cls;               // cls: zero-based class
  int32_t cx, cy, rx, ry, ellip;    // integer heat centre, radii, 1 = the elliptical Gaussian of an "outside" object
  int32_t x0, x1, y0, y1;           // heat window [x0, x1) x [y0, y1), clipped at the map border
  int32_t fr;                       // 1 = takes part in the frustum association
  int32_t roi_r0, roi_r1, roi_c0, roi_c1;   // radar ROI [r0, r1) x [c0, c1)
  int32_t p_r0, p_r1, p_c0, p_c1;           // paint rectangle
  double den_x, den_y;              // 2 * sigma^2 per axis
  double lo, hi;                    // depth gate: lo < v < hi
};
static_assert(sizeof(TgtDesc) == CF_TARGETS_DESC_BYTES, "cf_targets_workspace_bytes");

__device__ __forceinline__ float clipf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// utils/image.py:145-176 on Python ints (math.ceil of the box): float64 throughout, the reference's own (b + sq) / 2 roots
__device__ double gaussian_radius(int height, int width) {
  const double hh = (double)height, ww = (double)width, ov = 0.7;
  const double b1 = hh + ww;
  const double c1 = ww * hh * (1 - ov) / (1 + ov);
  const double r1 = (b1 + sqrt(b1 * b1 - 4 * 1 * c1)) / 2;
  const double b2 = 2 * (hh + ww);
  const double c2 = (1 - ov) * ww * hh;
  const double r2 = (b2 + sqrt(b2 * b2 - 4 * 4 * c2)) / 2;
  const double a3 = 4 * ov;
  const double b3 = -2 * ov * (hh + ww);
  const double c3 = (ov - 1) * ww * hh;
  const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
  return fmin(fmin(r1, r2), r3);
}

// utils/pointcloud.py:239-296 for one box: R (fp32) @ corners (fp32), fp32 products and sums as numpy's einsum forms them.
// xs / zs: rows 0 and 2 of the rotated corners; ys: the corner heights (row 1 passes through the 0 / 1 / 0 row unchanged).
__device__ void corners3d(double hdim, double wdim, double ldim, double yaw, float* xs, float* ys, float* zs) {
  const float c = (float)cos(yaw), s = (float)sin(yaw);
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float x = (float)((double)(((m >> 1) & 1) ? -0.5f : 0.5f) * ldim);
    const float y = m < 4 ? 0.0f : (float)(hdim * -1);
    const float z = (float)((double)((((m + 1) >> 1) & 1) ? -0.5f : 0.5f) * wdim);
    xs[m] = (c * x + 0.0f * y) + s * z;
    ys[m] = (0.0f * x + 1.0f * y) + 0.0f * z;
    zs[m] = ((-s) * x + 0.0f * y) + c * z;
  }
}

template <typename T>
__device__ __forceinline__ void put(T* p, size_t i, T v) {
  if (p) p[i] = v;
}

__global__ void __launch_bounds__(TGT_THREADS) targets_object_kernel(cf_targets_args a, TgtDesc* __restrict__ desc) {
  const int r = blockIdx.x * TGT_THREADS + threadIdx.x;
  if (r >= a.B * a.M) return;
  const int b = r / a.M, i = r - b * a.M;
  const double* an = a.ann + (size_t)r * CF_TARGETS_F;
  const int cid = a.iann[(size_t)r * 3 + 0], attr = a.iann[(size_t)r * 3 + 1], bits = a.iann[(size_t)r * 3 + 2];
  const double* T = a.trans + (size_t)b * 6;
  const int h = a.h, w = a.w;
  const bool rep3d = a.flags & CF_TARGETS_REP3D, norm2d = a.flags & CF_TARGETS_NORM2D;

  bool keep = i < a.counts[b] && !(cid > a.C || cid <= -999);          // generic_dataset.py:209-215

  // ---- transformBbox (generic_dataset.py:495-526): fp32 box, float64 transform stored to fp32, min / max, clip
  const float bx0 = (float)an[0], by0 = (float)an[1], bx1 = (float)(an[0] + an[2]), by1 = (float)(an[1] + an[3]);
  const float px[4] = {bx0, bx0, bx1, bx1}, py[4] = {by0, by1, by1, by0};
  float x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float tx = (float)(T[0] * (double)px[k] + T[1] * (double)py[k] + T[2] * 1.0);
    const float ty = (float)(T[3] * (double)px[k] + T[4] * (double)py[k] + T[5] * 1.0);
    x_lo = k ? fminf(x_lo, tx) : tx;
    x_hi = k ? fmaxf(x_hi, tx) : tx;
    y_lo = k ? fminf(y_lo, ty) : ty;
    y_hi = k ? fmaxf(y_hi, ty) : ty;
  }
  x_lo = clipf(x_lo, 0.0f, (float)(w - 1));
  x_hi = clipf(x_hi, 0.0f, (float)(w - 1));
  y_lo = clipf(y_lo, 0.0f, (float)(h - 1));
  y_hi = clipf(y_hi, 0.0f, (float)(h - 1));

  // ---- addInstance (generic_dataset.py:528-687)
  const float height = y_hi - y_lo, width = x_hi - x_lo;
  if (height <= 0 || width <= 0) keep = false;
  const float cx = (x_lo + x_hi) / 2.0f, cy = (y_lo + y_hi) / 2.0f;

  const bool has_amodal = bits & CF_TARGETS_HAS_AMODAL;
  double amx = 0, amy = 0;
  if (has_amodal) {                                                    // affineTransform stores the point to fp32 first
    const double ax = (double)(float)an[5], ay = (double)(float)an[6];
    amx = T[0] * ax + T[1] * ay + T[2] * 1.0;
    amy = T[3] * ax + T[4] * ay + T[5] * 1.0;
  }
  double hx = (double)cx, hy = (double)cy;
  bool outside = false;
  if (rep3d && has_amodal) {
    hx = clipd(amx, 0.0, (double)(w - 1));
    hy = clipd(amy, 0.0, (double)(h - 1));
    outside = !(hx == amx && hy == amy);
  }
  int rx, ry;
  if (outside) {
    rx = max(1, (int)(width * 0.5f));
    ry = max(1, (int)(height * 0.5f));
  } else {
    rx = ry = max(0, (int)gaussian_radius((int)ceilf(height), (int)ceilf(width)));
  }

  TgtDesc d;
  memset(&d, 0, sizeof(d));
  float o_bbox[4] = {0, 0, 0, 0}, o_center[2] = {0, 0}, o_heat[2] = {0, 0}, o_reg[2] = {0, 0}, o_amodal[2] = {0, 0};
  float o_wh[2] = {0, 0}, o_att[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o_attm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o_vel[3] = {0, 0, 0};
  float o_rotres[2] = {0, 0}, o_rot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o_depth = 0, o_dim[3] = {0, 0, 0}, o_trunc = 0;
  int64_t o_rotbin[2] = {0, 0};
  float c3x[8], c3y[8], c3z[8];
  bool has3d = false;

  if (keep) {
    o_trunc = (float)an[4];
    o_bbox[0] = x_lo, o_bbox[1] = y_lo, o_bbox[2] = x_hi, o_bbox[3] = y_hi;
    o_center[0] = cx, o_center[1] = cy;
    o_heat[0] = (float)hx, o_heat[1] = (float)hy;
    o_reg[0] = (float)((double)cx - hx), o_reg[1] = (float)((double)cy - hy);
    if (has_amodal) {
      o_amodal[0] = (float)(amx - hx), o_amodal[1] = (float)(amy - hy);
      if (norm2d) {
        o_amodal[0] = (float)((double)o_amodal[0] / (double)w);
        o_amodal[1] = (float)((double)o_amodal[1] / (double)h);
      }
    }
    o_wh[0] = norm2d ? width / (float)w : width;
    o_wh[1] = norm2d ? height / (float)h : height;
    if ((bits & CF_TARGETS_HAS_ATTRIBUTES) && attr > 0 && attr <= 8) {
      const int k = attr - 1, g0 = k < 2 ? 0 : k < 5 ? 2 : 5, g1 = k < 2 ? 2 : k < 5 ? 5 : 8;   // nuscenes.py:99-108
      o_att[k] = 1.0f;
      for (int g = g0; g < g1; ++g) o_attm[g] = 1.0f;
    }
    if ((bits & CF_TARGETS_HAS_VELOCITY) && an[10] > -1000) {
      o_vel[0] = (float)an[7], o_vel[1] = (float)an[8], o_vel[2] = (float)an[9];
    }
    if (a.flags & CF_TARGETS_WRITE_ROT) {
      const bool has_alpha = bits & CF_TARGETS_HAS_ALPHA;
      const double alpha = has_alpha ? an[11] : 0.0;
      o_rot[3] = 1.0f, o_rot[7] = 1.0f;                                // processAlpha (generic_dataset.py:689-708)
      if (alpha < TGT_PI / 6.0 || alpha > 5 * TGT_PI / 6.0) {
        const double rr = alpha - (-0.5 * TGT_PI);
        o_rot[1] = 1.0f, o_rot[2] = (float)sin(rr), o_rot[3] = (float)cos(rr);
        if (has_alpha) o_rotbin[0] = 1, o_rotres[0] = (float)rr;
      }
      if (alpha > -TGT_PI / 6.0 || alpha < -5 * TGT_PI / 6.0) {
        const double rr = alpha - (0.5 * TGT_PI);
        o_rot[5] = 1.0f, o_rot[6] = (float)sin(rr), o_rot[7] = (float)cos(rr);
        if (has_alpha) o_rotbin[1] = 1, o_rotres[1] = (float)rr;
      }
    }
    if ((bits & CF_TARGETS_HAS_DEPTH) && (a.flags & CF_TARGETS_WRITE_DEPTH)) o_depth = (float)(an[12] * a.scale[b]);
    if (bits & CF_TARGETS_HAS_DIMENSION) o_dim[0] = (float)an[13], o_dim[1] = (float)an[14], o_dim[2] = (float)an[15];
    const int need3d = CF_TARGETS_HAS_DIMENSION | CF_TARGETS_HAS_LOCATION | CF_TARGETS_HAS_YAW;
    if ((bits & need3d) == need3d) {                                    // get3dBox (utils/ddd.py:8-23)
      has3d = true;
      corners3d(an[13], an[14], an[15], an[19], c3x, c3y, c3z);
    }

    // ---- the descriptor: Gaussian window (utils/image.py:243-252) ...
    const int x = (int)hx, y = (int)hy;
    d.valid = 1, d.cls = cid - 1, d.cx = x, d.cy = y, d.rx = rx, d.ry = ry, d.ellip = outside ? 1 : 0;
    d.x0 = x - min(x, rx), d.x1 = x + min(w - x, rx + 1);
    d.y0 = y - min(y, ry), d.y1 = y + min(h - y, ry + 1);
    const double sgx = (double)(2 * rx + 1) / 6, sgy = (double)(2 * ry + 1) / 6;
    d.den_x = 2 * sgx * sgx, d.den_y = 2 * sgy * sgy;

    // ---- ... and the ground-truth frustum (getDistanceThresh, pointcloud.py:299-328; cvtPcDepthToHeatmap, 424-437, 466-476)
    if (a.flags & CF_TARGETS_FRUSTUM) {
      const float* cal = a.calib + (size_t)b * 12;
      const float yawf = (float)atan2((double)(cx - cal[2]), (double)cal[0]);      // np.arctan2 on fp32 operands
      double yaw = an[11] + (double)yawf;
      if (yaw > TGT_PI) yaw -= 2 * TGT_PI;
      if (yaw < -TGT_PI) yaw += 2 * TGT_PI;
      float gx[8], gy[8], gz[8];
      corners3d(an[13], an[14], an[15], yaw, gx, gy, gz);
      float zmax = gz[0], zmin = gz[0];
#pragma unroll
      for (int m = 1; m < 8; ++m) zmax = fmaxf(zmax, gz[m]), zmin = fminf(zmin, gz[m]);
      const float thr = zmax - zmin / 2.0f;                            // (the reference's own precedence)
      const float depth = (float)an[12];
      const float hi = depth + thr, lo = depth - thr;
      d.fr = 1, d.hi = (double)hi, d.lo = lo > 0 ? (double)lo : 0.0;
      py_slice((int)floorf(y_lo), (int)ceilf(y_hi) + 1, h, d.roi_r0, d.roi_r1);
      py_slice((int)floorf(x_lo), (int)ceilf(x_hi) + 1, w, d.roi_c0, d.roi_c1);
      const float wi = 0.3f * width, hi_ = 0.3f * height;
      py_slice((int)(cx - wi / 2.0f), (int)(cx + wi / 2.0f) + 1 + 1, w, d.p_c0, d.p_c1);
      py_slice((int)(cy - hi_ / 2.0f), (int)(cy + hi_ / 2.0f) + 1, h, d.p_r0, d.p_r1);
    }
  }
  desc[r] = d;

  const size_t R = (size_t)r;
  put(a.cls, R, (int64_t)(keep ? cid - 1 : 0));
  put(a.mask, R, keep ? 1.0f : 0.0f);
  put(a.trunc_mask, R, o_trunc);
  put(a.depth, R, o_depth);
  put(a.t_scores, R, 0.0f);
  for (int k = 0; k < 2; ++k) {
    put(a.wh, R * 2 + k, o_wh[k]);
    put(a.reg, R * 2 + k, o_reg[k]);
    put(a.amodal_offset, R * 2 + k, o_amodal[k]);
    put(a.rotbin, R * 2 + k, o_rotbin[k]);
    put(a.rotres, R * 2 + k, o_rotres[k]);
    put(a.t_centers, R * 2 + k, o_center[k]);
    put(a.t_heat_centers, R * 2 + k, o_heat[k]);
  }
  for (int k = 0; k < 3; ++k) {
    put(a.dimension, R * 3 + k, o_dim[k]);
    put(a.velocity, R * 3 + k, o_vel[k]);
    put(a.t_velocity, R * 3 + k, 0.0f);
  }
  for (int k = 0; k < 4; ++k) put(a.t_bboxes, R * 4 + k, o_bbox[k]);
  for (int k = 0; k < 8; ++k) {
    put(a.att, R * 8 + k, o_att[k]);
    put(a.att_mask, R * 8 + k, o_attm[k]);
    put(a.t_att, R * 8 + k, 0.0f);
    put(a.t_rotation, R * 8 + k, o_rot[k]);
  }
  if (a.t_bboxes3d) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      a.t_bboxes3d[R * 24 + m * 3 + 0] = has3d ? (float)((double)c3x[m] + an[16]) : 0.0f;
      a.t_bboxes3d[R * 24 + m * 3 + 1] = has3d ? (float)((double)c3y[m] + an[17]) : 0.0f;
      a.t_bboxes3d[R * 24 + m * 3 + 2] = has3d ? (float)((double)c3z[m] + an[18]) : 0.0f;
    }
  }
}

// ---- heat map: a workgroup per (row band, image); the image's descriptors staged in LDS, those that miss the band culled.
// drawGaussianHeatRegion (utils/image.py:179-256): the Gaussian in float64, the eps * max cut-off (max = 1: the window of the
// Gaussian matrix always holds its centre), rounded to fp32, np.maximum into the map.  A maximum: no order, the same bits each call.
__global__ void __launch_bounds__(TGT_THREADS) targets_heat_kernel(const TgtDesc* __restrict__ desc, float* __restrict__ heat, int M,
                                                                   int C, int h, int w) {
  __shared__ TgtDesc sd[CF_TARGETS_MAX_OBJS];
  __shared__ int s_list[CF_TARGETS_MAX_OBJS];
  __shared__ int s_n;
  const int b = blockIdx.y, y_lo = blockIdx.x * TGT_BAND, y_hi = min(h, y_lo + TGT_BAND);
  for (int j = threadIdx.x; j < M; j += TGT_THREADS) sd[j] = desc[(size_t)b * M + j];
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int j = 0; j < M; ++j) {
      const TgtDesc& d = sd[j];
      if (d.valid && d.cls >= 0 && d.cls < C && d.y0 < y_hi && d.y1 > y_lo && d.x0 < d.x1) s_list[n++] = j;
    }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n, rows = y_hi - y_lo, per_c = rows * w;
  for (int e = threadIdx.x; e < C * per_c; e += TGT_THREADS) {
    const int c = e / per_c, q = e - c * per_c;
    const int py = y_lo + q / w, px = q % w;
    float best = 0.0f;
    for (int k = 0; k < n; ++k) {
      const TgtDesc& d = sd[s_list[k]];
      if (d.cls != c || px < d.x0 || px >= d.x1 || py < d.y0 || py >= d.y1) continue;
      const double dx = (double)(px - d.cx), dy = (double)(py - d.cy);
      double v = d.ellip ? exp(-(dx * dx) / d.den_x - (dy * dy) / d.den_y) : exp(-(dx * dx + dy * dy) / d.den_x);
      if (v < 2.220446049250313e-16 * 1.0) v = 0.0;
      best = fmaxf(best, (float)v);
    }
    heat[(((size_t)b * C + c) * h + py) * w + px] = best;
  }
}

// ---- ground-truth frustum map (cvtPcDepthToHeatmap on numpy inputs, pointcloud.py:437-481): a workgroup per (row band, image).
// The boxes whose paint rectangle reaches the band are associated here, a wave per box: the first row-major minimum among the
// non-zero radar pixels of the ROI inside the depth gate.  Then every pixel of the band takes the LAST box in annotation order
// that has a hit and covers it - the order numpy's successive slice assignments leave - or zero.
__global__ void __launch_bounds__(TGT_THREADS) targets_frustum_kernel(const TgtDesc* __restrict__ desc, const float* __restrict__ pc_dep,
                                                                      float* __restrict__ pc_hm, int M, int h, int w, float max_pc_dist) {
  __shared__ TgtDesc sd[CF_TARGETS_MAX_OBJS];
  __shared__ int s_list[CF_TARGETS_MAX_OBJS];
  __shared__ float s_val[CF_TARGETS_MAX_OBJS][3];
  __shared__ int s_hit[CF_TARGETS_MAX_OBJS];
  __shared__ int s_n;
  const int b = blockIdx.y, y_lo = blockIdx.x * TGT_BAND, y_hi = min(h, y_lo + TGT_BAND);
  const size_t plane = (size_t)h * w;
  const float* dep = pc_dep + (size_t)b * 3 * plane;
  for (int j = threadIdx.x; j < M; j += TGT_THREADS) sd[j] = desc[(size_t)b * M + j];
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int j = 0; j < M; ++j) {
      const TgtDesc& d = sd[j];
      if (d.valid && d.fr && d.p_r0 < y_hi && d.p_r1 > y_lo && d.p_c0 < d.p_c1) s_list[n++] = j;
    }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < n; k += TGT_THREADS / 64) {
    const TgtDesc& d = sd[s_list[k]];
    const int cw = d.roi_c1 - d.roi_c0, cnt = cw > 0 && d.roi_r1 > d.roi_r0 ? (d.roi_r1 - d.roi_r0) * cw : 0;
    float best = 0.0f;
    int at = 0x7fffffff;
    for (int q = lane; q < cnt; q += 64) {
      const int rr = d.roi_r0 + q / cw, cc = d.roi_c0 + q % cw;
      const float v = dep[(size_t)rr * w + cc];
      if (v != 0.0f && (double)v < d.hi && (double)v > d.lo && (at == 0x7fffffff || v < best)) best = v, at = q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(at, off, 64);
      if (oa != 0x7fffffff && (at == 0x7fffffff || ov < best || (ov == best && oa < at))) best = ov, at = oa;
    }
    if (lane == 0) {
      s_hit[k] = at != 0x7fffffff;
      if (at != 0x7fffffff) {
        const size_t p = (size_t)(d.roi_r0 + at / cw) * w + (d.roi_c0 + at % cw);
        s_val[k][0] = best / max_pc_dist;
        s_val[k][1] = dep[plane + p];
        s_val[k][2] = dep[2 * plane + p];
      }
    }
  }
  __syncthreads();
  float* out = pc_hm + (size_t)b * 3 * plane;
  for (int e = threadIdx.x; e < (y_hi - y_lo) * w; e += TGT_THREADS) {
    const int py = y_lo + e / w, px = e % w;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    for (int k = n - 1; k >= 0; --k) {
      const TgtDesc& d = sd[s_list[k]];
      if (s_hit[k] && py >= d.p_r0 && py < d.p_r1 && px >= d.p_c0 && px < d.p_c1) {
        v0 = s_val[k][0], v1 = s_val[k][1], v2 = s_val[k][2];
        break;
      }
    }
    const size_t p = (size_t)py * w + px;
    out[p] = v0, out[plane + p] = v1, out[2 * plane + p] = v2;
  }
}

}  // namespace

extern "C" size_t cf_targets_workspace_bytes(int B, int M) {
  if (B <= 0 || M <= 0) return 0;
  return (size_t)B * (size_t)M * CF_TARGETS_DESC_BYTES;
}

extern "C" int cf_targets_build(const cf_targets_args* a, void* stream) {
  CF_REQUIRE(a, "cf_targets_build: null argument block");
  CF_REQUIRE(a->B > 0 && a->M > 0 && a->M <= CF_TARGETS_MAX_OBJS, "cf_targets_build: need B > 0 and 1 <= M <= %d (got B %d, M %d)",
             CF_TARGETS_MAX_OBJS, a->B, a->M);
  CF_REQUIRE(a->C > 0 && a->h > 0 && a->w > 0, "cf_targets_build: need C, h, w > 0");
  CF_REQUIRE((double)a->B * a->C * a->h * a->w < 2147483648.0 && a->B <= 65535, "cf_targets_build: B * C * h * w must stay below 2^31");
  CF_REQUIRE(a->ann && a->iann && a->counts && a->trans && a->scale, "cf_targets_build: null input table (ann, iann, counts, trans, scale)");
  CF_REQUIRE(a->heat && a->cls && a->mask && a->trunc_mask && a->wh && a->t_bboxes && a->t_centers && a->t_heat_centers &&
                 a->t_bboxes3d && a->t_scores,
             "cf_targets_build: null output among heat, cls, mask, trunc_mask, wh, t_bboxes, t_centers, t_heat_centers, t_bboxes3d, t_scores");
  CF_REQUIRE(!(a->rotbin || a->rotres || a->t_rotation) || (a->rotbin && a->rotres && a->t_rotation),
             "cf_targets_build: rotbin, rotres and t_rotation come together");
  CF_REQUIRE(!a->att == !a->att_mask, "cf_targets_build: att and att_mask come together");
  const bool frustum = a->flags & CF_TARGETS_FRUSTUM;
  CF_REQUIRE(!frustum || (a->pc_dep && a->pc_hm && a->calib && a->max_pc_dist > 0),
             "cf_targets_build: CF_TARGETS_FRUSTUM needs pc_dep, pc_hm, calib and max_pc_dist > 0");
  CF_REQUIRE(a->workspace && a->workspace_bytes >= cf_targets_workspace_bytes(a->B, a->M),
             "cf_targets_build: workspace of %zu bytes, need %zu", a->workspace_bytes, cf_targets_workspace_bytes(a->B, a->M));
  hipStream_t st = (hipStream_t)stream;
  TgtDesc* desc = (TgtDesc*)a->workspace;
  const int rows = a->B * a->M;
  targets_object_kernel<<<dim3((rows + TGT_THREADS - 1) / TGT_THREADS), dim3(TGT_THREADS), 0, st>>>(*a, desc);
  int rc = cf_check_launch("cf_targets_build (objects)");
  if (rc) return rc;
  const dim3 grid((a->h + TGT_BAND - 1) / TGT_BAND, a->B);
  targets_heat_kernel<<<grid, dim3(TGT_THREADS), 0, st>>>(desc, a->heat, a->M, a->C, a->h, a->w);
  rc = cf_check_launch("cf_targets_build (heat map)");
  if (rc) return rc;
  if (frustum) {
    targets_frustum_kernel<<<grid, dim3(TGT_THREADS), 0, st>>>(desc, a->pc_dep, a->pc_hm, a->M, a->h, a->w, a->max_pc_dist);
    rc = cf_check_launch("cf_targets_build (frustum map)");
  }
  return rc;
}
