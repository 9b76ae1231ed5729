// In front of the network: image preprocessing, radar ingest and the expansion of radar points into the pc_dep map
// (pillars / points / heatmap).  Float64 and fixed-point arithmetic written operation for operation like the reference's
// (numpy, OpenCV); this file is compiled with -ffp-contract=off so no multiply-add is fused behind our back.
#include "cf_common.h"
#include "cf_warp_u8.h"

namespace {
constexpr int PL_THREADS = 256;
constexpr int PL_MAXN = 1024;
constexpr int PL_MAX_CELLS = (96 * 1024) / 4;   // 96 KiB of rank map per workgroup
// METHOD (DATASET.PC_ROI_METHOD, generic_dataset.py:774-826): 0 = "pillars", 1 = "points" (drawPcPoints, nuscenes.py:265-294: the one
// pixel the truncated coordinates name; of several points on a pixel the last in order stays, as the rank map has it),
// 2 = "heatmap" (a square of the Gaussian radius of a (250 / depth + 5)-sized object around the truncated centre).
constexpr int ROI_PILLARS = 0, ROI_POINTS = 1, ROI_HEATMAP = 2;
constexpr int RI_MAXN = 1024;

// ---------------------------------------------------------------------------------------------
// Pillar expansion (dataset/generic_dataset.py:738-942, datasets/nuscenes.py:221-263), fp64
// ---------------------------------------------------------------------------------------------
struct PlBox {
  int y0, y1, x0, x1;
  float d, vx, vz;
};

// utils/image.py:145-176 (getGaussianRadius((r, r), min_overlap = 0.7)) in float64, operation by operation
__device__ __forceinline__ double gaussian_radius_sq(double r) {
  const double mo = 0.7;
  const double height = r, width = r;
  const double b1 = height + width;
  const double c1 = width * height * (1 - mo) / (1 + mo);
  const double sq1 = sqrt(b1 * b1 - 4 * 1 * c1);
  const double r1 = (b1 + sq1) / 2;
  const double b2 = 2 * (height + width);
  const double c2 = (1 - mo) * width * height;
  const double sq2 = sqrt(b2 * b2 - 4 * 4 * c2);
  const double r2 = (b2 + sq2) / 2;
  const double a3 = 4 * mo;
  const double b3 = -2 * mo * (height + width);
  const double c3 = (mo - 1) * width * height;
  const double sq3 = sqrt(b3 * b3 - 4 * a3 * c3);
  const double r3 = (b3 + sq3) / 2;
  return fmin(fmin(r1, r2), r3);
}

// One workgroup per frame.  (1) per-point fp64 geometry -> integer box; (2) LDS rank map: every kept
// point atomicMax-es its depth rank over its rectangle, a wave per point (points are depth-ascending,
// painting order = rank order, so the surviving value of a pixel is that of its highest rank);
// (3) resolve ranks to (depth, vx, vz).  The rank map is processed in row bands that fit LDS.
template <int METHOD>
__global__ __launch_bounds__(PL_THREADS) void pillar_kernel(
    const double* __restrict__ pc_2d, const double* __restrict__ pc_3d, const int32_t* __restrict__ counts,
    int max_n, int n_rows, const double* __restrict__ calib, const double* __restrict__ trans, int H, int W,
    double ph, double pw, double pl, float* __restrict__ pc_dep, uint8_t* __restrict__ keep_mask,
    double* __restrict__ xy_out, int band_rows) {
  extern __shared__ __attribute__((aligned(16))) int rank_map[];  // band_rows * W
  __shared__ PlBox box[PL_MAXN];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = counts[b];
  const double* p2 = pc_2d + (size_t)b * 3 * max_n;
  const double* p3 = pc_3d + (size_t)b * n_rows * max_n;
  const double* cal = calib + (size_t)b * 12;
  const double* m = trans + (size_t)b * 6;

  for (int i = tid; i < max_n; i += PL_THREADS) {
    PlBox bx;
    bx.y0 = bx.y1 = bx.x0 = bx.x1 = 0;
    bx.d = bx.vx = bx.vz = 0.0f;
    bool keep = false;
    double tx = 0.0, ty = 0.0;
    if (i < n) {
      const double u = p2[i], v = p2[max_n + i];
      tx = m[0] * u + m[1] * v + m[2];
      ty = m[3] * u + m[4] * v + m[5];
      keep = (tx < (double)W) && (ty < (double)H) && (0.0 < tx) && (0.0 < ty);
      if (keep && METHOD == ROI_POINTS) {
        const int x = (int)tx, y = (int)ty;              // astype(np.int32): truncation (0 < tx < W, 0 < ty < H)
        py_slice(y, y + 1, H, bx.y0, bx.y1);
        py_slice(x, x + 1, W, bx.x0, bx.x1);
      } else if (keep && METHOD == ROI_HEATMAP) {
        const double depth = p2[2 * (size_t)max_n + i];
        double rad = gaussian_radius_sq((1.0 / depth) * 250 + 5);
        if (!(rad < 1048576.0)) rad = 1048576.0;         // (depth -> 0: far beyond any map; the min() below clip it)
        const int radius = max(0, (int)rad);
        const int x = (int)tx, y = (int)ty;
        const int left = min(x, radius), right = min(W - x, radius + 1);
        const int top = min(y, radius), bottom = min(H - y, radius + 1);
        py_slice(y - top, y + bottom, H, bx.y0, bx.y1);
        py_slice(x - left, x + right, W, bx.x0, bx.x1);
      }
      if (keep && METHOD != ROI_PILLARS) {
        bx.d = (float)p2[2 * (size_t)max_n + i];
        bx.vx = (float)p3[8 * (size_t)max_n + i];
        bx.vz = (float)p3[9 * (size_t)max_n + i];
      }
      if (keep && METHOD == ROI_PILLARS) {
        // 8 corners of the (h,w,l) pillar standing on the point, yaw 0; corner offsets are float32
        // in the reference (numpy float32 arrays), the sum with the fp64 location is fp64.
        const double X = p3[i], Y = p3[max_n + i], Z = p3[2 * (size_t)max_n + i];
        const double ox = (double)(float)(0.5 * pl), oz = (double)(float)(0.5 * pw);
        const double oy = (double)(float)(-ph);
        double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        for (int q = 0; q < 8; ++q) {
          const double cxq = X + ((q & 3) < 2 ? ox : -ox);
          const double cyq = Y + (q < 4 ? 0.0 : oy);
          const double czq = Z + (((q & 3) == 0 || (q & 3) == 3) ? oz : -oz);
          const double pu = ((cal[0] * cxq + cal[1] * cyq) + cal[2] * czq) + cal[3];
          const double pv = ((cal[4] * cxq + cal[5] * cyq) + cal[6] * czq) + cal[7];
          const double pz = ((cal[8] * cxq + cal[9] * cyq) + cal[10] * czq) + cal[11];
          const double uu = pu / pz, vv = pv / pz;
          const double ou = m[0] * uu + m[1] * vv + m[2];
          const double ov = m[3] * uu + m[4] * vv + m[5];
          xmin = fmin(xmin, ou); xmax = fmax(xmax, ou);
          ymin = fmin(ymin, ov); ymax = fmax(ymax, ov);
        }
        const double bw = xmax - xmin, bh = ymax - ymin;
        const double y1 = fmax(ty - bh, 0.0), y2 = ty;
        const double x1 = fmax(tx - bw / 2, 0.0), x2 = fmin(tx + bw / 2, (double)W);
        // np.round == round-half-to-even == rint; then numpy slicing clips to the map
        int iy0 = (int)rint(y1), iy1 = (int)rint(y2), ix0 = (int)rint(x1), ix1 = (int)rint(x2);
        py_slice(iy0, iy1, H, bx.y0, bx.y1);
        py_slice(ix0, ix1, W, bx.x0, bx.x1);
        bx.d = (float)p2[2 * (size_t)max_n + i];
        bx.vx = (float)p3[8 * (size_t)max_n + i];
        bx.vz = (float)p3[9 * (size_t)max_n + i];
      }
    }
    if (!keep) bx.y1 = bx.y0 = 0;
    if (i < PL_MAXN) box[i] = bx;
    if (keep_mask) keep_mask[(size_t)b * max_n + i] = keep ? 1 : 0;
    if (xy_out) {
      xy_out[((size_t)b * 2 + 0) * max_n + i] = tx;
      xy_out[((size_t)b * 2 + 1) * max_n + i] = ty;
    }
  }
  __syncthreads();

  float* out = pc_dep + (size_t)b * 3 * H * W;
  const int HW = H * W;
  for (int r0 = 0; r0 < H; r0 += band_rows) {
    const int r1 = min(r0 + band_rows, H);
    const int cells = (r1 - r0) * W;
    for (int i = tid; i < cells; i += PL_THREADS) rank_map[i] = -1;
    __syncthreads();
    for (int i = wave; i < n; i += PL_THREADS / 64) {
      const PlBox bx = box[i];
      const int ya = max(bx.y0, r0), yb = min(bx.y1, r1);
      const int rw = bx.x1 - bx.x0;
      if (yb <= ya || rw <= 0) continue;
      const int cnt = (yb - ya) * rw;
      for (int q = lane; q < cnt; q += 64) {
        const int yy = ya + q / rw, xx = bx.x0 + q % rw;
        atomicMax(&rank_map[(yy - r0) * W + xx], i);
      }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += PL_THREADS) {
      const int rk = rank_map[i];
      float d = 0.0f, vx = 0.0f, vz = 0.0f;
      if (rk >= 0) {
        d = box[rk].d;
        vx = box[rk].vx;
        vz = box[rk].vz;
      }
      const int p = r0 * W + i;
      out[p] = d;
      out[HW + p] = vx;
      out[2 * HW + p] = vz;
    }
    __syncthreads();
  }
}

// the checks, the row band and the launch of one pillar_kernel form (`who`: the entry point that was called)
template <int METHOD>
int pillar_launch(const char* who, const double* pc_2d, const double* pc_3d, const int32_t* counts, int B, int max_n,
                  int n_rows, const double* calib, const double* trans, int H, int W, double ph, double pw, double pl,
                  float* pc_dep, uint8_t* keep_mask, double* xy_out, void* stream) {
  CF_REQUIRE(pc_2d && pc_3d && counts && calib && trans && pc_dep, "%s: null buffer", who);
  CF_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  CF_REQUIRE(max_n >= 1 && max_n <= PL_MAXN, "%s: max_n=%d outside [1,%d]", who, max_n, PL_MAXN);
  CF_REQUIRE(n_rows >= 10, "%s: pc_3d needs >= 10 rows (8 = vx, 9 = vz)", who);
  const int band_rows = (long)H * W > PL_MAX_CELLS ? PL_MAX_CELLS / W : H;
  CF_REQUIRE(band_rows >= 1, "%s: W=%d too wide", who, W);
  const size_t lds = (size_t)band_rows * W * sizeof(int);
  static CfLdsLimit lds_limit;
  lds_limit.ensure(pillar_kernel<METHOD>, lds, 65536);
  hipLaunchKernelGGL(pillar_kernel<METHOD>, dim3(B), dim3(PL_THREADS), lds, (hipStream_t)stream, pc_2d, pc_3d, counts,
                     max_n, n_rows, calib, trans, H, W, ph, pw, pl, pc_dep, keep_mask, xy_out, band_rows);
  return cf_check_launch(who);
}
}  // namespace

extern "C" int cf_pillar_expand(const double* pc_2d, const double* pc_3d, const int32_t* counts, int B,
                                int max_n, int n_rows, const double* calib, const double* trans, int H, int W,
                                double pillar_h, double pillar_w, double pillar_l, float* pc_dep,
                                uint8_t* keep_mask, double* xy_out, void* stream) {
  return pillar_launch<ROI_PILLARS>("cf_pillar_expand", pc_2d, pc_3d, counts, B, max_n, n_rows, calib, trans, H, W, pillar_h,
                                    pillar_w, pillar_l, pc_dep, keep_mask, xy_out, stream);
}

// DATASET.PC_ROI_METHOD "points" / "heatmap" (method 1 / 2; 0 = pillars with the reference's default pillar): the inputs and
// outputs of cf_pillar_expand, the same rank-map painting.
extern "C" int cf_radar_roi_expand(const double* pc_2d, const double* pc_3d, const int32_t* counts, int B, int max_n,
                                   int n_rows, const double* calib, const double* trans, int H, int W, int method,
                                   float* pc_dep, uint8_t* keep_mask, double* xy_out, void* stream) {
  CF_REQUIRE(method == ROI_POINTS || method == ROI_HEATMAP,
             "cf_radar_roi_expand: method=%d (1 = points, 2 = heatmap; pillars: cf_pillar_expand)", method);
  const auto launch = method == ROI_POINTS ? pillar_launch<ROI_POINTS> : pillar_launch<ROI_HEATMAP>;
  return launch("cf_radar_roi_expand", pc_2d, pc_3d, counts, B, max_n, n_rows, calib, trans, H, W, 0.0, 0.0, 0.0, pc_dep,
                keep_mask, xy_out, stream);
}

namespace {
// ---------------------------------------------------------------------------------------------
// Radar ingest (detector.py:257-283, nuscenes.py:171-199, pointcloud.py:17-49):
// raw sweep (R rows x N points, float64, camera frame) -> depth gate, y offset, pinhole projection,
// image-border gate, depth order -> the padded pc_2d / pc_3d / counts that cf_pillar_expand consumes.
// One workgroup per frame, one thread per point; the order is a rank by counting over LDS
// (depth, then original index: a stable sort; N <= 1024 so N^2 comparisons are a few microseconds).
// Arithmetic order as oracle/radar_ref.py fixes it (products summed left to right, no FMA).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RI_MAXN) void radar_ingest_kernel(
    const double* __restrict__ pc, const int32_t* __restrict__ counts_in, int R, int max_n,
    const double* __restrict__ intr, double width, double height, double max_dist, double z_offset,
    int descending, double* __restrict__ pc_2d, double* __restrict__ pc_3d, int32_t* __restrict__ counts_out) {
  __shared__ double s_depth[RI_MAXN];
  __shared__ int s_keep[RI_MAXN];
  __shared__ int s_total;
  const int b = blockIdx.x, i = threadIdx.x;
  const int n = min(counts_in[b], max_n);
  const double* src = pc + (size_t)b * R * max_n;
  const double* K = intr + (size_t)b * 9;
  if (i == 0) s_total = 0;
  bool keep = false;
  double u = 0.0, v = 0.0, z = 0.0, y = 0.0;
  if (i < n) {
    const double x = src[i];
    y = src[(size_t)max_n + i];
    z = src[(size_t)2 * max_n + i];
    keep = !(max_dist > 0.0) || z <= max_dist;
    if (z_offset != 0.0) y -= z_offset;
    const double px = K[0] * x + K[1] * y + K[2] * z;
    const double py = K[3] * x + K[4] * y + K[5] * z;
    const double pz = K[6] * x + K[7] * y + K[8] * z;
    u = px / pz;
    v = py / pz;
    keep = keep && z > 0.0 && u > 1.0 && u < width - 1.0 && v > 1.0 && v < height - 1.0;
  }
  s_depth[i] = z;
  s_keep[i] = keep ? 1 : 0;
  __syncthreads();
  if (keep) {
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double dj = s_depth[j];
      rank += (s_keep[j] && (dj < z || (dj == z && j < i))) ? 1 : 0;
    }
    atomicAdd(&s_total, 1);
    s_keep[i] = rank + 1;                  // (every thread has read s_keep[i] only as a flag: still non-zero)
  }
  __syncthreads();
  const int total = s_total;
  if (i == 0) counts_out[b] = total;
  double* o2 = pc_2d + (size_t)b * 3 * max_n;
  double* o3 = pc_3d + (size_t)b * R * max_n;
  if (keep) {
    const int rank = s_keep[i] - 1;
    const int pos = descending ? total - 1 - rank : rank;
    o2[pos] = u;
    o2[(size_t)max_n + pos] = v;
    o2[(size_t)2 * max_n + pos] = z;
    for (int r = 0; r < R; ++r) o3[(size_t)r * max_n + pos] = (r == 1) ? y : src[(size_t)r * max_n + i];
  }
  // zero the padding so the output is fully defined
  for (int j = total + i; j < max_n; j += RI_MAXN) {
    o2[j] = 0.0; o2[(size_t)max_n + j] = 0.0; o2[(size_t)2 * max_n + j] = 0.0;
    for (int r = 0; r < R; ++r) o3[(size_t)r * max_n + j] = 0.0;
  }
}
}  // namespace

extern "C" int cf_radar_ingest(const double* pc, const int32_t* counts_in, int B, int n_rows, int max_n,
                               const double* intrinsics, int img_w, int img_h, double max_dist, double z_offset,
                               int descending, double* pc_2d, double* pc_3d, int32_t* counts_out, void* stream) {
  CF_REQUIRE(pc && counts_in && intrinsics && pc_2d && pc_3d && counts_out, "cf_radar_ingest: null buffer");
  CF_REQUIRE(B > 0 && n_rows >= 3 && img_w > 2 && img_h > 2, "cf_radar_ingest: bad geometry");
  CF_REQUIRE(max_n >= 1 && max_n <= RI_MAXN, "cf_radar_ingest: max_n=%d outside [1,%d]", max_n, RI_MAXN);
  hipLaunchKernelGGL(radar_ingest_kernel, dim3(B), dim3(RI_MAXN), 0, (hipStream_t)stream, pc, counts_in, n_rows,
                     max_n, intrinsics, (double)img_w, (double)img_h, max_dist, z_offset, descending, pc_2d, pc_3d,
                     counts_out);
  return cf_check_launch("cf_radar_ingest");
}

namespace {
// ---------------------------------------------------------------------------------------------
// Image side of Detector.pre_process (detector.py:226-234): cv2.warpAffine(INTER_LINEAR, constant
// border 0) of the uint8 camera frame in OpenCV's fixed-point arithmetic (10-bit coordinates, 5-bit
// bilinear fractions, 15-bit weights: oracle/preprocess_ref.py states it), then
// ((v / 255.0 - mean) / std) in float64 -> fp32, HWC -> CHW.  One thread per output pixel.
// (The warp itself is cf_warp_affine_u8, cf_warp_u8.h, shared with the training warp of cf_augment.hip.)
// ---------------------------------------------------------------------------------------------
struct PreK {
  const uint8_t* src;   // (B, Hs, Ws, 3)
  float* out;           // (B, 3, Hd, Wd)
  double m[6];          // dst -> src map (already inverted)
  double mean[3], stdv[3];
  int B, Hs, Ws, Hd, Wd;
};

__global__ __launch_bounds__(256) void preprocess_kernel(PreK p) {
  const long total = (long)p.B * p.Hd * p.Wd;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % p.Wd);
    const long r = i / p.Wd;
    const int y = (int)(r % p.Hd), b = (int)(r / p.Hd);
    int v[3];
    cf_warp_affine_u8(p.src + (size_t)b * p.Hs * p.Ws * 3, p.Hs, p.Ws, p.m, x, y, false, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double n = ((double)v[c] / 255.0 - p.mean[c]) / p.stdv[c];
      p.out[(((size_t)b * 3 + c) * p.Hd + y) * p.Wd + x] = (float)n;
    }
  }
}
}  // namespace

extern "C" int cf_preprocess_images(const uint8_t* src, int B, int Hs, int Ws, const double* map_dst_to_src,
                                    const float* mean, const float* stdv, int Hd, int Wd, float* out, void* stream) {
  CF_REQUIRE(src && map_dst_to_src && mean && stdv && out, "cf_preprocess_images: null buffer");
  CF_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "cf_preprocess_images: bad geometry");
  CF_REQUIRE(Hs < 32768 && Ws < 32768 && Hd < 32768 && Wd < 32768, "cf_preprocess_images: image too large for the fixed-point map");
  PreK k{};
  k.src = src; k.out = out;
  for (int i = 0; i < 6; ++i) k.m[i] = map_dst_to_src[i];        // host memory: six doubles
  for (int c = 0; c < 3; ++c) {
    CF_REQUIRE(stdv[c] != 0.0f, "cf_preprocess_images: std[%d] is zero", c);
    k.mean[c] = (double)mean[c];
    k.stdv[c] = (double)stdv[c];
  }
  k.B = B; k.Hs = Hs; k.Ws = Ws; k.Hd = Hd; k.Wd = Wd;
  const long total = (long)B * Hd * Wd;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, k);
  return cf_check_launch("cf_preprocess_images");
}
