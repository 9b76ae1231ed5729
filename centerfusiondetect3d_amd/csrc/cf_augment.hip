// Training inputs on the device (reference dataset/generic_dataset.py:414-439 transformInput with its colorAugmentor, and the
// img[:, ::-1, :] of :168): per frame an affine warp with the frame's own matrix, optionally of the mirrored source, then the
// torchvision chain ToTensor -> RandomOrder(ColorJitter brightness / contrast / saturation) -> lightingAug -> Normalize in fp32,
// HWC uint8 -> CHW fp32.  Semantics: include/cf_hip.h (cf_augment_images); CPU statement: tests/train_inputs_ref.py.
//
// Built with -ffp-contract=off: every fp32 operation of the chain rounds on its own, as torch's CPU kernels do.
//
// Contrast blends with the mean grey level of the WHOLE frame as it stands at that point of the chain, so with `colour` there
// are two launches:
//   augment_stats_kernel   warps each pixel once, stashes the three bytes (uchar4, in the workspace), runs the chain up to the
//                          contrast step and adds up the grey level in float64: one partial sum per 1024-pixel block.
//   augment_finish_kernel  adds the frame's partial sums (every block does, in the same fixed order), reads the stash, runs the
//                          whole chain and writes the three planes.
// No atomics: the partition of a frame into blocks, the order inside a block and the order over the partials depend on Hd * Wd
// alone, so a frame's bits do not depend on the run or on the batch it is in.  Without `colour` the finish kernel warps itself
// and nothing else is launched.
#include "cf_common.h"
#include "cf_warp_u8.h"

namespace {
constexpr int AUG_THREADS = 256;
constexpr int AUG_PX = 1024;          // output pixels per block (4 per thread); one float64 partial sum per block
enum { AUG_BRIGHTNESS = 0, AUG_CONTRAST = 1, AUG_SATURATION = 2 };   // values of `order`: the reference's ColorJitter list

struct AugK {
  const uint8_t* src;        // (B, Hs, Ws, 3)
  float* out;                // (B, 3, Hd, Wd)
  const double* map;         // (B, 6) dst -> src
  const uint8_t* flip;       // (B)
  const int32_t* order;      // (B, 3)
  const float* factor;       // (B, 3), indexed by the operation
  const float* lighting;     // (B, 3)
  double* partial;           // (B, nblk)
  uchar4* stash;             // (B, Hd * Wd)
  float mean[3], stdv[3];
  int Hs, Ws, Hd, Wd, nblk;  // nblk: blocks per frame
};

// The jitter parameters of one frame, uniform over a block.
struct AugChain {
  int order[3];
  float r[3], q[3];          // per position: the factor and (float)(1 - (double)factor), as torchvision's _blend forms them
};

__device__ __forceinline__ AugChain aug_chain(const AugK& p, int b) {
  AugChain ch;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int k = p.order[b * 3 + i];
    const bool ok = (unsigned)k < 3u;                    // (the host validates the table; a bad entry is a no-op, not a wild read)
    ch.order[i] = ok ? k : -1;
    ch.r[i] = ok ? p.factor[b * 3 + k] : 1.0f;
    ch.q[i] = (float)(1.0 - (double)ch.r[i]);
  }
  return ch;
}

__device__ __forceinline__ float aug_blend(float r, float q, float a, float o) {
  return fminf(fmaxf(r * a + q * o, 0.0f), 1.0f);
}

__device__ __forceinline__ float aug_grey(const float (&t)[3]) {
  return (0.2989f * t[0] + 0.587f * t[1]) + 0.114f * t[2];
}

// step `i` of the chain on one pixel; `m`: the frame's mean grey level (read by the contrast step only)
__device__ __forceinline__ void aug_step(const AugChain& ch, int i, float (&t)[3], float m) {
  const int k = ch.order[i];
  if (k < 0) return;
  const float o = k == AUG_BRIGHTNESS ? 0.0f : (k == AUG_CONTRAST ? m : aug_grey(t));
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = aug_blend(ch.r[i], ch.q[i], t[c], o);
}

// Sum over the block in a fixed order (lanes by halving, then the four waves); every thread gets the result.
__device__ __forceinline__ double aug_block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return s;
}

__device__ __forceinline__ void aug_load_map(const AugK& p, int b, double (&m)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) m[i] = p.map[(size_t)b * 6 + i];
}

__global__ __launch_bounds__(AUG_THREADS) void augment_stats_kernel(AugK p) {
  __shared__ double lds[AUG_THREADS / 64];
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int n = p.Hd * p.Wd;
  double m[6];
  aug_load_map(p, b, m);
  const bool mirror = p.flip[b] != 0;
  const AugChain ch = aug_chain(p, b);
  int before = 3;                                        // the steps in front of the contrast
#pragma unroll
  for (int i = 2; i >= 0; --i) before = ch.order[i] == AUG_CONTRAST ? i : before;
  const uint8_t* img = p.src + (size_t)b * p.Hs * p.Ws * 3;
  uchar4* stash = p.stash + (size_t)b * n;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < AUG_PX / AUG_THREADS; ++j) {
    const int i = blk * AUG_PX + j * AUG_THREADS + (int)threadIdx.x;
    if (i >= n) break;
    int v[3];
    cf_warp_affine_u8(img, p.Hs, p.Ws, m, i % p.Wd, i / p.Wd, mirror, v);
    stash[i] = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], 0);
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = __fdiv_rn((float)v[c], 255.0f);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (s < before) aug_step(ch, s, t, 0.0f);
    acc += (double)aug_grey(t);
  }
  const double s = aug_block_sum(acc, lds);
  if (threadIdx.x == 0) p.partial[(size_t)b * p.nblk + blk] = s;
}

template <bool COLOUR>
__global__ __launch_bounds__(AUG_THREADS) void augment_finish_kernel(AugK p) {
  __shared__ double lds[AUG_THREADS / 64];
  const int b = (int)(blockIdx.x / (unsigned)p.nblk), blk = (int)(blockIdx.x % (unsigned)p.nblk);
  const int n = p.Hd * p.Wd;
  double m[6];
  bool mirror = false;
  AugChain ch;
  float grey_mean = 0.0f, light[3] = {0.0f, 0.0f, 0.0f};
  if (COLOUR) {
    ch = aug_chain(p, b);
    double a = 0.0;
    for (int i = (int)threadIdx.x; i < p.nblk; i += AUG_THREADS) a += p.partial[(size_t)b * p.nblk + i];
    grey_mean = (float)(aug_block_sum(a, lds) / (double)n);          // float64 sum / n, rounded once
#pragma unroll
    for (int c = 0; c < 3; ++c) light[c] = p.lighting[b * 3 + c];
  } else {
    aug_load_map(p, b, m);
    mirror = p.flip[b] != 0;
  }
  const uint8_t* img = p.src + (size_t)b * p.Hs * p.Ws * 3;
  const uchar4* stash = p.stash + (size_t)b * n;
  float* out = p.out + (size_t)b * 3 * n;
#pragma unroll
  for (int j = 0; j < AUG_PX / AUG_THREADS; ++j) {
    const int i = blk * AUG_PX + j * AUG_THREADS + (int)threadIdx.x;
    if (i >= n) break;
    int v[3];
    if (COLOUR) {
      const uchar4 s = stash[i];
      v[0] = s.x; v[1] = s.y; v[2] = s.z;
    } else {
      cf_warp_affine_u8(img, p.Hs, p.Ws, m, i % p.Wd, i / p.Wd, mirror, v);
    }
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = __fdiv_rn((float)v[c], 255.0f);
    if (COLOUR) {
#pragma unroll
      for (int s = 0; s < 3; ++s) aug_step(ch, s, t, grey_mean);
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] += light[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(size_t)c * n + i] = __fdiv_rn(t[c] - p.mean[c], p.stdv[c]);
  }
}

inline long aug_blocks_per_frame(int Hd, int Wd) { return ((long)Hd * Wd + AUG_PX - 1) / AUG_PX; }
}  // namespace

extern "C" size_t cf_augment_workspace_bytes(int B, int Hd, int Wd) {
  if (B <= 0 || Hd <= 0 || Wd <= 0) return 0;
  return (size_t)B * (size_t)aug_blocks_per_frame(Hd, Wd) * sizeof(double) + (size_t)B * Hd * Wd * sizeof(uchar4);
}

extern "C" int cf_augment_images(const uint8_t* src, int B, int Hs, int Ws, const double* map_dst_to_src, const uint8_t* flip,
                                 const int32_t* order, const float* factor, const float* lighting, const float* mean,
                                 const float* stdv, int colour, int Hd, int Wd, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  CF_REQUIRE(src && map_dst_to_src && flip && mean && stdv && out, "cf_augment_images: null buffer");
  CF_REQUIRE(!colour || (order && factor && lighting), "cf_augment_images: colour needs order, factor and lighting");
  CF_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "cf_augment_images: bad geometry");
  CF_REQUIRE(Hs < 32768 && Ws < 32768 && Hd < 32768 && Wd < 32768, "cf_augment_images: image too large for the fixed-point map");
  const long nblk = aug_blocks_per_frame(Hd, Wd);
  CF_REQUIRE((long)B * nblk <= 0x7fffffffL, "cf_augment_images: B * ceil(Hd * Wd / %d) = %ld blocks exceeds the grid limit 2^31 - 1",
             AUG_PX, (long)B * nblk);
  AugK k{};
  for (int c = 0; c < 3; ++c) {
    CF_REQUIRE(stdv[c] != 0.0f, "cf_augment_images: std[%d] is zero", c);
    k.mean[c] = mean[c];
    k.stdv[c] = stdv[c];
  }
  if (colour) {
    CF_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "cf_augment_images: colour needs an 8-byte aligned workspace");
    CF_REQUIRE(workspace_bytes >= cf_augment_workspace_bytes(B, Hd, Wd), "cf_augment_images: workspace of %zu bytes, %zu needed",
               workspace_bytes, cf_augment_workspace_bytes(B, Hd, Wd));
    k.partial = (double*)workspace;
    k.stash = (uchar4*)(k.partial + (size_t)B * nblk);
  }
  k.src = src; k.out = out; k.map = map_dst_to_src; k.flip = flip; k.order = order; k.factor = factor; k.lighting = lighting;
  k.Hs = Hs; k.Ws = Ws; k.Hd = Hd; k.Wd = Wd; k.nblk = (int)nblk;
  const dim3 grid((unsigned)((long)B * nblk)), block(AUG_THREADS);
  if (colour) {
    hipLaunchKernelGGL(augment_stats_kernel, grid, block, 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(augment_finish_kernel<true>, grid, block, 0, (hipStream_t)stream, k);
  } else {
    hipLaunchKernelGGL(augment_finish_kernel<false>, grid, block, 0, (hipStream_t)stream, k);
  }
  return cf_check_launch("cf_augment_images");
}
