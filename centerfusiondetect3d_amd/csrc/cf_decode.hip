// Behind the peaks: detection gather (decode), 2D -> 3D postProcess, the Detector's depth maps and the nuScenes result
// serialisation.  One thread per detection (or per pixel); the arithmetic is written operation for operation like the
// reference's, and this file is compiled with -ffp-contract=off so no multiply-add is fused behind our back.
#include "cf_common.h"

#define DM_THREADS 1024

namespace {
constexpr int SR_THREADS = 256;
constexpr int SR_MAXC = 6144;   // candidates per sample (6 cameras x K <= 1024)

// ---------------------------------------------------------------------------------------------
// Detection gather (model/decode.py:40-41, 60-64, 132-172)
// ---------------------------------------------------------------------------------------------
// `unc`: the (B,1,H,W) map of the `uncertainty` head or NULL.  With it the score WRITTEN to the row is
// score * exp(-exp(u)) at the peak pixel (model/decode.py:80-85, precise expf); a.scores is only read, so the
// peak buffers the forward may share between decodes keep the raw scores, and the row order stays the top-K's.
__device__ __forceinline__ void decode_row(const cf_decode_args& a, const float* __restrict__ unc, int t, float* o) {
  const int b = t / a.K;
  const int HW = a.H * a.W;
  const int pix = a.inds[t];
  const int yi = pix / a.W, xi = pix - yi * a.W;
  const float xn = (float)xi / (float)a.W, yn = (float)yi / (float)a.H;
  const float score = a.scores[t];
  o[0] = unc ? score * expf(-expf(unc[(size_t)b * HW + pix])) : score;
  o[1] = (float)a.classes[t];
  o[2] = xn;
  o[3] = yn;
  const float xf = xn * (float)a.out_w, yf = yn * (float)a.out_h;
  float xc, yc;
  if (a.reg) {
    xc = xf + a.reg[((size_t)b * 2 + 0) * HW + pix];
    yc = yf + a.reg[((size_t)b * 2 + 1) * HW + pix];
  } else {
    xc = xf + 0.5f;
    yc = yf + 0.5f;
  }
  const float sx = a.norm2d ? (float)a.out_w : 1.0f, sy = a.norm2d ? (float)a.out_h : 1.0f;
  if (a.wh) {
    float w = a.wh[((size_t)b * 2 + 0) * HW + pix], h = a.wh[((size_t)b * 2 + 1) * HW + pix];
    w = (w < 0.0f ? 0.0f : w) * sx;
    h = (h < 0.0f ? 0.0f : h) * sy;
    o[4] = xc - w / 2.0f;
    o[5] = yc - h / 2.0f;
    o[6] = xc + w / 2.0f;
    o[7] = yc + h / 2.0f;
  } else {
    o[4] = o[5] = o[6] = o[7] = 0.0f;
  }
  auto gather = [&](const float* m, int nc, int off, float s0, float s1) {
    for (int c = 0; c < nc; ++c) {
      float v = m ? m[((size_t)b * nc + c) * HW + pix] : 0.0f;
      if (m) v *= (c == 0 ? s0 : (c == 1 ? s1 : 1.0f));
      o[off + c] = v;
    }
  };
  gather(a.rot, 8, 8, 1.0f, 1.0f);
  gather(a.dim, 3, 16, 1.0f, 1.0f);
  gather(a.amodal, 2, 19, sx, sy);
  gather(a.att, 8, 21, 1.0f, 1.0f);
  gather(a.vel, 3, 29, 1.0f, 1.0f);
  gather(a.depth, 1, 32, 1.0f, 1.0f);
}

__global__ void decode_gather_kernel(cf_decode_args a, const float* __restrict__ unc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.B * a.K) return;
  decode_row(a, unc, t, a.det + (size_t)t * 33);
}
}  // namespace

// (one launcher for both forms: `unc` NULL = the plain decode)
static int decode_gather_launch(const char* who, const cf_decode_args* a, const float* unc, void* stream) {
  CF_REQUIRE(a && a->scores && a->inds && a->classes && a->det, "%s: null buffer", who);
  CF_REQUIRE(a->B > 0 && a->K > 0 && a->H > 0 && a->W > 0, "%s: bad geometry", who);
  const int n = a->B * a->K;
  hipLaunchKernelGGL(decode_gather_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, *a, unc);
  return cf_check_launch(who);
}

extern "C" int cf_decode_gather(const cf_decode_args* a, void* stream) {
  return decode_gather_launch("cf_decode_gather", a, nullptr, stream);
}

extern "C" int cf_decode_gather_unc(const cf_decode_args* a, const float* uncertainty, void* stream) {
  CF_REQUIRE(uncertainty, "cf_decode_gather_unc: null uncertainty map");
  return decode_gather_launch("cf_decode_gather_unc", a, uncertainty, stream);
}

namespace {
// ---------------------------------------------------------------------------------------------
// 2D -> 3D post-processing of decoded detections (utils/postProcess.py:13-85), one thread per row.
// in : det (B,K,33) [score, cls, cxn, cyn, x1, y1, x2, y2, rot8, dim3, amodal2, att8, vel3, depth]
// out: (B,K,54) [score, cls+1, cx, cy, x1, y1, x2, y2, depth, alpha, dim3, amodal2, att8, vel3,
//                loc3, yaw, box3d 8x3]
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void post_row(const float* d, const float* __restrict__ cal,
                                         const float* __restrict__ tinv, float out_w, float out_h, float* o) {
  const float t00 = tinv[0], t01 = tinv[1], t02 = tinv[2], t10 = tinv[3], t11 = tinv[4], t12 = tinv[5];
  auto ax = [&](float x, float y) { return (t00 * x + t01 * y) + t02; };
  auto ay = [&](float x, float y) { return (t10 * x + t11 * y) + t12; };
  o[0] = d[0];
  o[1] = d[1] + 1.0f;
  // 2D boxes back to the source image
  o[4] = ax(d[4], d[5]); o[5] = ay(d[4], d[5]);
  o[6] = ax(d[6], d[7]); o[7] = ay(d[6], d[7]);
  const float depth = d[32];
  o[8] = depth;
  // observation angle (pointcloud.py:207-210)
  const float* r = d + 8;
  const float idx = r[1] > r[5] ? 1.0f : 0.0f;
  const float a1 = atan2f(r[2], r[3]) + (float)(-0.5 * M_PI);
  const float a2 = atan2f(r[6], r[7]) + (float)(0.5 * M_PI);
  const float alpha = a1 * idx + a2 * (1.0f - idx);
  o[9] = alpha;
  const float dh = d[16], dw = d[17], dl = d[18];
  o[10] = dh; o[11] = dw; o[12] = dl;
  o[13] = d[19]; o[14] = d[20];
  for (int i = 0; i < 8; ++i) o[15 + i] = d[21 + i];
  // centre = affine(normalised centre * (W,H) + amodal offset)
  const float px = d[2] * out_w + d[19], py = d[3] * out_h + d[20];
  const float cx = ax(px, py), cy = ay(px, py);
  o[2] = cx; o[3] = cy;
  // unproject (ddd.py:143-166) and yaw (ddd.py:122-140)
  const float z = depth - cal[11];
  const float X = ((cx * depth - cal[3]) - cal[2] * z) / cal[0];
  const float Y = ((cy * depth - cal[7]) - cal[6] * z) / cal[5] + dh / 2.0f;
  float yaw = alpha + atan2f(cx - cal[2], cal[0]);
  const float PI_F = (float)M_PI, TWO_PI_F = (float)(2.0 * M_PI);
  if (yaw > PI_F) yaw -= TWO_PI_F;
  if (yaw < -PI_F) yaw += TWO_PI_F;
  o[26] = X; o[27] = Y; o[28] = z;
  o[29] = yaw;
  // velocity re-projected on the heading
  const float cs = cosf(yaw), sn = sinf(yaw);
  const float V = sqrtf(d[29] * d[29] + d[31] * d[31]);
  o[23] = cs * V; o[24] = d[30]; o[25] = -sn * V;
  // 3D box corners (pointcloud.py:239-296 + ddd.py:8-23); zero if any dimension <= 0
  const bool bad = dh <= 0.0f || dw <= 0.0f || dl <= 0.0f;
  const float hx = 0.5f * dl, hz = 0.5f * dw;
  const float sx[4] = {hx, hx, -hx, -hx}, sz[4] = {hz, -hz, -hz, hz};
  for (int q = 0; q < 8; ++q) {
    const float xc = sx[q & 3], yc = q < 4 ? 0.0f : -dh, zc = sz[q & 3];
    const float bx = ((cs * xc + 0.0f * yc) + sn * zc) + X;
    const float by = ((0.0f * xc + 1.0f * yc) + 0.0f * zc) + Y;
    const float bz = (((-sn) * xc + 0.0f * yc) + cs * zc) + z;
    o[30 + q * 3 + 0] = bad ? 0.0f : bx;
    o[30 + q * 3 + 1] = bad ? 0.0f : by;
    o[30 + q * 3 + 2] = bad ? 0.0f : bz;
  }
}

__global__ void post_process_kernel(const float* __restrict__ det, const float* __restrict__ calib,
                                    const float* __restrict__ tinv, int B, int K, float out_w, float out_h,
                                    float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * K) return;
  post_row(det + (size_t)t * 33, calib + (size_t)(t / K) * 12, tinv, out_w, out_h, out + (size_t)t * 54);
}
}  // namespace

extern "C" int cf_post_process(const float* det, const float* calib, const float* trans_inv, int B, int K,
                               int out_h, int out_w, float* out, void* stream) {
  CF_REQUIRE(det && calib && trans_inv && out, "cf_post_process: null buffer");
  CF_REQUIRE(B > 0 && K > 0 && out_h > 0 && out_w > 0, "cf_post_process: bad geometry");
  const int n = B * K;
  hipLaunchKernelGGL(post_process_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, det, calib,
                     trans_inv, B, K, (float)out_w, (float)out_h, out);
  return cf_check_launch("cf_post_process");
}

namespace {
// decode + postProcess in ONE launch: the 33-float row stays in registers between the two steps
// (model/decode.py:10-174 -> utils/postProcess.py:13-85); `a.det` may be NULL when only the final rows
// are wanted.  Same arithmetic as the two kernels above (this file is built without FMA contraction),
// so the fused rows equal cf_decode_gather + cf_post_process bit for bit.
__global__ void decode_post_kernel(cf_decode_args a, const float* __restrict__ unc, const float* __restrict__ calib,
                                   const float* __restrict__ tinv, float* __restrict__ post) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.B * a.K) return;
  float d[33];
  decode_row(a, unc, t, d);
  if (a.det) {
    float* o = a.det + (size_t)t * 33;
#pragma unroll
    for (int i = 0; i < 33; ++i) o[i] = d[i];
  }
  post_row(d, calib + (size_t)(t / a.K) * 12, tinv, (float)a.out_w, (float)a.out_h, post + (size_t)t * 54);
}
}  // namespace

static int decode_post_launch(const char* who, const cf_decode_args* a, const float* unc, const float* calib,
                              const float* trans_inv, float* post, void* stream) {
  CF_REQUIRE(a && a->scores && a->inds && a->classes && calib && trans_inv && post, "%s: null buffer", who);
  CF_REQUIRE(a->B > 0 && a->K > 0 && a->H > 0 && a->W > 0 && a->out_h > 0 && a->out_w > 0, "%s: bad geometry", who);
  const int n = a->B * a->K;
  hipLaunchKernelGGL(decode_post_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, *a, unc, calib,
                     trans_inv, post);
  return cf_check_launch(who);
}

extern "C" int cf_decode_post(const cf_decode_args* a, const float* calib, const float* trans_inv, float* post,
                             void* stream) {
  return decode_post_launch("cf_decode_post", a, nullptr, calib, trans_inv, post, stream);
}

extern "C" int cf_decode_post_unc(const cf_decode_args* a, const float* uncertainty, const float* calib,
                                 const float* trans_inv, float* post, void* stream) {
  CF_REQUIRE(uncertainty, "cf_decode_post_unc: null uncertainty map");
  return decode_post_launch("cf_decode_post_unc", a, uncertainty, calib, trans_inv, post, stream);
}

namespace {
// ---------------------------------------------------------------------------------------------
// Normalised uint8 depth maps of Detector.post_process (detector.py:381-393), all maps of a batch in one launch:
// one workgroup per (image, map).  Pass 1: min / max over the image's H*W values, row 0 and column 0 of IMAGE 0 read
// as 0 (the reference's `depthmap[0, 0] = 0; depthmap[0, :, 0] = 0` indexes the batch, not the map: kept); wave
// reduction, then LDS across the waves.  Pass 2 (the map is in L2 by then): ((x - min) / (max - min)) * 255 truncated,
// each operation rounded on its own (this file is built without FMA contraction; the division is IEEE), which is
// numpy's result bit for bit.  A flat image gives 0 / 0: defined as 0 here (numpy's cast of NaN is not defined).
// V = 4: W % 4 == 0 and 16-byte-aligned maps - float4 loads, one 4-byte store per lane; V = 1: any shape.
// ---------------------------------------------------------------------------------------------
struct DepthMapPtrs {
  const float* p[CF_DEPTH_MAPS_MAX];
  long stride[CF_DEPTH_MAPS_MAX];   // floats between two images of map m (H*W, or more for a channel view)
};

__device__ __forceinline__ unsigned char depth_u8(float x, float lo, float range) {
  const float f = ((x - lo) / range) * 255.0f;
  return f == f ? (unsigned char)(int)f : (unsigned char)0;
}

template <int V>
__global__ __launch_bounds__(DM_THREADS) void depth_maps_kernel(DepthMapPtrs maps, int B, int H, int W,
                                                                unsigned char* __restrict__ out) {
  const int b = blockIdx.x, m = blockIdx.y;
  const int HW = H * W, n = HW / V;
  const float* __restrict__ x = maps.p[m] + (size_t)b * maps.stride[m];
  unsigned char* __restrict__ o = out + ((size_t)m * B + b) * HW;
  const bool edge = b == 0;
  // element i of the image with the reference's zeroing applied (V = 4: a vector starts a row only at its lane 0)
  auto load = [&](int i, float* v) {
    if (V == 4) {
      const f32x4 q = reinterpret_cast<const f32x4*>(x)[i];
      const int e = i * 4;
      const bool row0 = edge && e < W;
      v[0] = (row0 || (edge && e % W == 0)) ? 0.0f : q[0];
      v[1] = row0 ? 0.0f : q[1];
      v[2] = row0 ? 0.0f : q[2];
      v[3] = row0 ? 0.0f : q[3];
    } else {
      const float q = x[i];
      v[0] = (edge && (i < W || i % W == 0)) ? 0.0f : q;
    }
  };
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < n; i += DM_THREADS) {
    float v[V];
    load(i, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      lo = fminf(lo, v[j]);
      hi = fmaxf(hi, v[j]);
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, s, 64));
    hi = fmaxf(hi, __shfl_xor(hi, s, 64));
  }
  __shared__ float red[2][DM_THREADS / 64];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lo;
    red[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < DM_THREADS / 64; ++w) {
    lo = fminf(lo, red[0][w]);
    hi = fmaxf(hi, red[1][w]);
  }
  const float range = hi - lo;
  for (int i = threadIdx.x; i < n; i += DM_THREADS) {
    float v[V];
    load(i, v);
    if (V == 4) {
      const unsigned int packed = (unsigned int)depth_u8(v[0], lo, range) | ((unsigned int)depth_u8(v[1], lo, range) << 8) |
                                  ((unsigned int)depth_u8(v[2], lo, range) << 16) |
                                  ((unsigned int)depth_u8(v[3], lo, range) << 24);
      reinterpret_cast<unsigned int*>(o)[i] = packed;
    } else {
      o[i] = depth_u8(v[0], lo, range);
    }
  }
}
}  // namespace

extern "C" int cf_depth_maps(const float* const* maps, const long* batch_strides, int n_maps, int B, int H, int W,
                             uint8_t* out, void* stream) {
  CF_REQUIRE(maps, "cf_depth_maps: null maps");
  CF_REQUIRE(out, "cf_depth_maps: null out");
  CF_REQUIRE(n_maps >= 1 && n_maps <= CF_DEPTH_MAPS_MAX, "cf_depth_maps: n_maps=%d (1..%d)", n_maps, CF_DEPTH_MAPS_MAX);
  CF_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W <= (1L << 30), "cf_depth_maps: bad geometry");
  DepthMapPtrs p = {};
  bool wide = W % 4 == 0 && (uintptr_t)out % 4 == 0;
  for (int m = 0; m < n_maps; ++m) {
    CF_REQUIRE(maps[m], "cf_depth_maps: null maps[%d]", m);
    p.p[m] = maps[m];
    p.stride[m] = batch_strides ? batch_strides[m] : (long)H * W;
    CF_REQUIRE(p.stride[m] >= (long)H * W, "cf_depth_maps: batch_strides[%d]=%ld < H*W", m, p.stride[m]);
    wide = wide && (uintptr_t)maps[m] % 16 == 0 && p.stride[m] % 4 == 0;
  }
  hipLaunchKernelGGL(wide ? depth_maps_kernel<4> : depth_maps_kernel<1>, dim3(B, n_maps), dim3(DM_THREADS), 0,
                     (hipStream_t)stream, p, B, H, W, out);
  return cf_check_launch("cf_depth_maps");
}

namespace {
// ---------------------------------------------------------------------------------------------
// nuScenes result serialisation (dataset/datasets/nuscenes.py:416-557)
// rows (B*K, 12) f32: [translation xyz (global), size w l h, velocity xy (global), score,
//                      class index 0..9, attribute id 0..8, keep]
// rotation (B*K, 4) f64: pose * cs * R_y(yaw)   (w, x, y, z)
// One thread per detection.  fp32 products of the 4x4 transforms are summed pairwise
// ((p0 + p1) + (p2 + p3)), each operation rounded - the order oracle/serialize_ref.py pins.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot4_pairwise(const float* m, float x, float y, float z, float w) {
  return (m[0] * x + m[1] * y) + (m[2] * z + m[3] * w);
}

__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

__global__ void serialize_rows_kernel(const float* __restrict__ post, int B, int K,
                                      const float* __restrict__ trans_matrix,
                                      const float* __restrict__ velocity_matrix,
                                      const double* __restrict__ cs_rot, const double* __restrict__ pose_rot,
                                      float* __restrict__ rows, double* __restrict__ rotation) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * K) return;
  const int b = t / K;
  const float* p = post + (size_t)t * 54;
  const float* tm = trans_matrix + (size_t)b * 16;
  const float* vm = velocity_matrix + (size_t)b * 16;
  float* o = rows + (size_t)t * 12;
  const float score = p[0];
  const int cls = (int)p[1] - 1;                          // classIds were shifted to 1..10 by postProcess
  const float dh = p[10], dw = p[11], dl = p[12];
  // size = dimension[[1, 2, 0]] = (w, l, h); location.y -= h in Python floats (fp64), then fp32
  const float lx = p[26], lz = p[28];
  const float ly = (float)((double)p[27] - (double)dh);
  o[0] = dot4_pairwise(tm + 0, lx, ly, lz, 1.0f);
  o[1] = dot4_pairwise(tm + 4, lx, ly, lz, 1.0f);
  o[2] = dot4_pairwise(tm + 8, lx, ly, lz, 1.0f);
  o[3] = dw; o[4] = dl; o[5] = dh;
  o[6] = dot4_pairwise(vm + 0, p[23], p[24], p[25], 0.0f);
  o[7] = dot4_pairwise(vm + 4, p[23], p[24], p[25], 0.0f);
  o[8] = score;
  o[9] = (float)cls;
  // attribute: argmax (first maximum) over the class group's slice of nuscenes_att (nuscenes.py:446-454)
  const float* att = p + 15;
  int attr = 0;
  if (cls == 6 || cls == 7) {                             // motorcycle, bicycle
    attr = (att[1] > att[0] ? 1 : 0) + 1;
  } else if (cls == 5) {                                  // pedestrian
    int m = 2;
    if (att[3] > att[m]) m = 3;
    if (att[4] > att[m]) m = 4;
    attr = (m - 2) + 3;
  } else if (cls >= 0 && cls <= 4) {                      // car, truck, bus, trailer, construction_vehicle
    int m = 5;
    if (att[6] > att[m]) m = 6;
    if (att[7] > att[m]) m = 7;
    attr = (m - 5) + 6;
  }
  o[10] = (float)attr;
  // merge filter of model/progressBar.py:116 / detector.py:437: score > -1 and every dimension > 0
  o[11] = (score > -1.0f && dh > 0.0f && dw > 0.0f && dl > 0.0f) ? 1.0f : 0.0f;
  if (rotation) {
    double* q = rotation + (size_t)t * 4;
    const double half = (double)p[29] / 2.0;
    const double ry[4] = {cos(half), 0.0, sin(half), 0.0};
    double tmp[4];
    if (cs_rot && pose_rot) {
      quat_mul(cs_rot + (size_t)b * 4, ry, tmp);
      quat_mul(pose_rot + (size_t)b * 4, tmp, q);
    } else {
      q[0] = ry[0]; q[1] = ry[1]; q[2] = ry[2]; q[3] = ry[3];
    }
  }
}

// Per-sample merge of the cameras' results + top-N cut (convert_eval_format, nuscenes.py:536-553):
// candidates = kept rows of the sample's frames in (frame order, row order); order = stable sort on
// the score, descending (Python sorts (-score, position)); the best `max_keep` survive.
// One workgroup per sample; rank by counting over the candidate list in LDS.
__global__ __launch_bounds__(SR_THREADS) void serialize_topn_kernel(
    const float* __restrict__ rows, int K, const int32_t* __restrict__ sample_ptr,
    const int32_t* __restrict__ sample_frames, int max_keep, int32_t* __restrict__ order,
    int32_t* __restrict__ counts) {
  __shared__ float s_score[SR_MAXC];
  __shared__ int s_row[SR_MAXC];
  __shared__ int s_wave[SR_THREADS / 64];
  __shared__ int s_base;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = sample_ptr[s], f1 = sample_ptr[s + 1];
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int f = f0; f < f1; ++f) {
    const int b = sample_frames[f];
    for (int j0 = 0; j0 < K; j0 += SR_THREADS) {
      const int j = j0 + tid;
      const int row = b * K + j;
      const bool keep = j < K && rows[(size_t)row * 12 + 11] != 0.0f;
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) s_wave[wave] = __popcll(bal);
      __syncthreads();
      int off = s_base;
      for (int w = 0; w < wave; ++w) off += s_wave[w];
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      if (keep && pos < SR_MAXC) {
        s_score[pos] = rows[(size_t)row * 12 + 8];
        s_row[pos] = row;
      }
      __syncthreads();
      if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < SR_THREADS / 64; ++w) tot += s_wave[w];
        s_base += tot;
      }
      __syncthreads();
    }
  }
  const int n = min(s_base, SR_MAXC);
  const int kept = min(n, max_keep);
  if (tid == 0) counts[s] = kept;
  for (int i = tid; i < n; i += SR_THREADS) {
    const float si = s_score[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s_score[j];
      rank += (sj > si || (sj == si && j < i)) ? 1 : 0;
    }
    if (rank < max_keep) order[(size_t)s * max_keep + rank] = s_row[i];
  }
  for (int i = kept + tid; i < max_keep; i += SR_THREADS) order[(size_t)s * max_keep + i] = -1;
}
}  // namespace

extern "C" int cf_serialize_nuscenes(const cf_serialize_args* a, void* stream) {
  CF_REQUIRE(a && a->post && a->trans_matrix && a->velocity_matrix && a->rows, "cf_serialize_nuscenes: null buffer");
  CF_REQUIRE(a->B > 0 && a->K > 0 && a->K <= 1024, "cf_serialize_nuscenes: bad geometry (K <= 1024)");
  CF_REQUIRE((a->cs_rot == nullptr) == (a->pose_rot == nullptr), "cf_serialize_nuscenes: cs_rot and pose_rot go together");
  const int n = a->B * a->K;
  hipLaunchKernelGGL(serialize_rows_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, a->post, a->B,
                     a->K, a->trans_matrix, a->velocity_matrix, a->cs_rot, a->pose_rot, a->rows, a->rotation);
  if (a->n_samples > 0) {
    CF_REQUIRE(a->sample_ptr && a->sample_frames && a->order && a->counts, "cf_serialize_nuscenes: null sample tables");
    CF_REQUIRE(a->max_per_sample >= 1, "cf_serialize_nuscenes: max_per_sample=%d", a->max_per_sample);
    hipLaunchKernelGGL(serialize_topn_kernel, dim3(a->n_samples), dim3(SR_THREADS), 0, (hipStream_t)stream, a->rows,
                       a->K, a->sample_ptr, a->sample_frames, a->max_per_sample, a->order, a->counts);
  }
  return cf_check_launch("cf_serialize_nuscenes");
}

extern "C" int cf_serialize_max_candidates(void) { return SR_MAXC; }
