// Training path of one detection head on a frozen trunk: conv3x3(Cin -> 256) + bias -> ReLU -> [conv1x1(256 -> 256) + bias -> ReLU] x n
// -> conv1x1(256 -> Cout) + bias, forward and backward, from the RAW fp32 weights (nothing packed is kept: the optimiser rewrites
// them every step).  The eval kernel (cf_heads.hip) is not involved.
//
// Both directions work on a LIST of pixels, chunk by chunk: the forward on all B*h*w pixels, the backward on the pixels where any
// channel of dY is non-zero (compacted on the device; the work loops read the device-side count, grids come from shapes, the host
// never waits).  Per chunk the hidden maps live in the caller's workspace as [chunk][256] rows; the backward RECOMPUTES them with
// the very kernel the forward ran (head_gemm_kernel: same products, same K order per element), so its ReLU mask is the forward's
// bit for bit.  ReLU'(0) = 0.
//
// Products on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulation; the small output layer on the VALU (fmaf).
// Weight / bias gradients are summed over pixel slabs with float atomics, and the compaction orders the list with an atomic
// counter: gradients can differ in their last bits from run to run.  The forward has neither and is bitwise reproducible.
//
// dX is produced on request only (cf_head_backward_dx; cf_head_backward serves a frozen trunk and launches nothing for it): at the
// end of each chunk the masked gradient of the first layer's pre-activation is multiplied with the 3x3 weights and scattered from
// the list to the nine neighbours of each pixel with float atomics (head_dgrad_kernel), into maps zeroed once per call - like
// gw / gb, gx / gx2 can differ in their last bits from run to run.
#include "cf_common.h"

namespace {

constexpr int HID = 256;           // hidden width (config.head_conv: 256 everywhere)
constexpr int GEMM_PX = 32;        // pixels per tile of head_gemm_kernel (one 32x32 MFMA row block)
constexpr int SLAB_PX = 256;       // pixels per slab of the weight-gradient kernels
constexpr int DEFAULT_CHUNK = 32768;
constexpr int GEMM_NT = 2;         // 32-output tiles per wave of head_gemm_kernel (grid.y = HID / (32 * GEMM_NT))
constexpr int KU = 4;              // MFMA k-steps (2 values of K each) whose loads are issued ahead of their MFMAs

struct HeadSrc {
  const float* x;
  const float* x2;                 // second source (channels cx .. cx + cx2 - 1) or null
  int xs, cx, x2s, cx2;
  int h, w;
};

// (begin, end) of this chunk's part of the list
__device__ __forceinline__ int list_end(const int* count, int M, int begin, int chunk) {
  const int n = count ? min(*count, M) : M;
  return min(n, begin + chunk);
}

struct HGemm {
  HeadSrc s;           // TAPS == 9: the rows are gathered from the image (zero rows outside it)
  const float* a;      // TAPS == 1: chunk-local rows [chunk][HID]
  const float* wk;     // [TAPS][K][HID]: K-major weights
  const float* bias;   // mode 0: out = ReLU(acc + bias)
  const float* mask;   // mode 1: out = mask > 0 ? acc : 0   (chunk-local [chunk][HID])
  float* out;          // chunk-local [chunk][HID]
  const int* idx;      // list (null: position q is pixel q)
  const int* count;    // device-side length of the list (null: M)
  int M, begin, chunk, K, mode;
  int kvec;            // leading channels of a row read as 16-byte vectors: a multiple of 16, 0 unless the rows are 16-byte aligned
};

// One wave = 32 list positions x 32 * GEMM_NT outputs: D[pixel][o] += A[pixel][k] B[k][o], two k per MFMA; every address is clamped into
// its tensor, so the loads are unconditional and what is not wanted is selected away.
template <int TAPS>
__global__ __launch_bounds__(64) void head_gemm_kernel(const HGemm p) {
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const int o0 = blockIdx.y * (32 * GEMM_NT);
  const int K = p.K;
  const int hw = p.s.h * p.s.w;
  for (int q0 = p.begin + blockIdx.x * GEMM_PX; q0 < end; q0 += gridDim.x * GEMM_PX) {
    const int q = q0 + cl;
    const bool live = q < end;
    f32x16 acc[GEMM_NT];
#pragma unroll
    for (int t = 0; t < GEMM_NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    int pb = 0, py = 0, px = 0;
    if (TAPS == 9) {
      const int pix = live ? (p.idx ? p.idx[q] : q) : 0;
      pb = pix / hw;
      const int rem = pix - pb * hw;
      py = rem / p.s.w;
      px = rem - py * p.s.w;
    }
    for (int tap = 0; tap < TAPS; ++tap) {
      const float* r0;
      const float* r1;
      bool ok = live;
      if (TAPS == 9) {
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        ok = live && yy >= 0 && yy < p.s.h && xx >= 0 && xx < p.s.w;
        const size_t row = ok ? (size_t)(pb * p.s.h + yy) * p.s.w + xx : 0;
        r0 = p.s.x + row * p.s.xs;
        r1 = p.s.x2 ? p.s.x2 + row * p.s.x2s : r0;
      } else {
        r0 = r1 = p.a + (size_t)(live ? q - p.begin : 0) * HID;
      }
      const int cx = TAPS == 9 ? p.s.cx : K;
      const float* wrow = p.wk + (size_t)tap * K * HID + o0 + cl;
      // the first kvec channels (a multiple of 16, rows 16-byte aligned) of the row as two 16-byte loads per lane: half 0 holds
      // channels k0 .. k0 + 3 (and + 8), half 1 the four behind them, so MFMA step s pairs channel k0 + s with k0 + 4 + s
      for (int k0 = 0; k0 < p.kvec; k0 += 16) {
        f32x4 a4[2];
        float bw[2][4][GEMM_NT];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int kb = k0 + 8 * v + 4 * half;
          a4[v] = *reinterpret_cast<const f32x4*>(r0 + kb);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < GEMM_NT; ++t) bw[v][s][t] = wrow[(size_t)(kb + s) * HID + 32 * t];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < GEMM_NT; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? a4[v][s] : 0.0f, bw[v][s][t], acc[t], 0, 0, 0);
      }
      for (int k0 = p.kvec; k0 < K; k0 += 2 * KU) {
        float av[KU], bv[KU][GEMM_NT];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          const int kk = k0 + 2 * u + half;
          const bool kin = kk < K;
          const int kc = kin ? kk : K - 1;
          const float* ap = kc < cx ? r0 + kc : r1 + (kc - cx);
          const float a = *ap;
          av[u] = (ok && kin) ? a : 0.0f;
#pragma unroll
          for (int t = 0; t < GEMM_NT; ++t) {
            const float b = wrow[(size_t)kc * HID + 32 * t];
            bv[u][t] = kin ? b : 0.0f;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
          for (int t = 0; t < GEMM_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][t], acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < GEMM_NT; ++t) {
      const int o = o0 + 32 * t + cl;
      const float bias = p.mode == 0 ? p.bias[o] : 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (qq < end) {
          const size_t li = (size_t)(qq - p.begin) * HID + o;
          float v = acc[t][r];
          if (p.mode == 0) {
            v += bias;
            v = v > 0.0f ? v : 0.0f;
          } else {
            v = p.mask[li] > 0.0f ? v : 0.0f;
          }
          p.out[li] = v;
        }
      }
    }
  }
}

struct HWgrad {
  HeadSrc s;           // TAPS == 9
  const float* a;      // TAPS == 1: chunk-local hidden map [chunk][HID] (the layer's input)
  const float* g;      // chunk-local gradient of the layer's pre-activation [chunk][HID]
  float* gw;           // element (o, c, tap) at o * ostride + c * cstride + tap; float atomics
  float* gb;           // [HID]; float atomics
  const int* idx;
  const int* count;
  int M, begin, chunk, K, ostride, cstride;
};

// One wave = one (pixel slab, tap, 32-channel chunk of the layer's input, 128 outputs): D[o][c] += g[pixel][o] in[pixel][c], two
// pixels per MFMA (the layout of dcn_bwd_weight_kernel).  The waves of tap 0, channel chunk 0 also add up g: the slab's part of gb.
template <int TAPS>
__global__ __launch_bounds__(64) void head_wgrad_kernel(const HWgrad p) {
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const int qb = p.begin + blockIdx.x * SLAB_PX;
  const int qe = min(end, qb + SLAB_PX);
  if (qb >= qe) return;
  const int nch = (p.K + 31) >> 5;
  const int tap = blockIdx.y / nch, ch = blockIdx.y - tap * nch;
  const int o0 = blockIdx.z * 128;
  const int c = ch * 32 + cl;
  const bool cin = c < p.K;
  const int cc = cin ? c : p.K - 1;
  const int hw = p.s.h * p.s.w;
  f32x16 acc[4];
  float bsum[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    bsum[t] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  }
  for (int q2 = qb; q2 < qe; q2 += 2 * KU) {
    float a[KU][4], col[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int q = q2 + 2 * u + half;
      const bool live = q < qe;
      const int qc = live ? q : qe - 1;
      const size_t lr = (size_t)(qc - p.begin) * HID;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float v = p.g[lr + o0 + 32 * t + cl];
        a[u][t] = live ? v : 0.0f;
      }
      if (TAPS == 9) {
        const int pix = p.idx ? p.idx[qc] : qc;
        const int pb = pix / hw, rem = pix - pb * hw;
        const int py = rem / p.s.w, px = rem - py * p.s.w;
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        const bool ok = live && cin && yy >= 0 && yy < p.s.h && xx >= 0 && xx < p.s.w;
        const size_t row = ok ? (size_t)(pb * p.s.h + yy) * p.s.w + xx : 0;
        const float* sp = (cc < p.s.cx || !p.s.x2) ? p.s.x + row * p.s.xs + min(cc, p.s.cx - 1) : p.s.x2 + row * p.s.x2s + (cc - p.s.cx);
        const float v = *sp;
        col[u] = ok ? v : 0.0f;
      } else {
        const float v = p.a[lr + cc];
        col[u] = (live && cin) ? v : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) bsum[t] += a[u][t];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], col[u], acc[t], 0, 0, 0);
  }
  if (cin) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
        atomicAdd(p.gw + (size_t)o * p.ostride + (size_t)c * p.cstride + tap, acc[t][r]);
      }
  }
  if (blockIdx.y == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);
      if (half == 0) atomicAdd(p.gb + o0 + 32 * t + cl, v);
    }
  }
}

// dst[(tap * K + c) * HID + o] = src[(o * K + c) * T + tap]: the raw (256, K, T) weight, K-major
__global__ __launch_bounds__(256) void head_wk_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int T) {
  const int n = T * K * HID;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int o = i & (HID - 1), kc = i >> 8;
    const int tap = kc / K, c = kc - tap * K;
    dst[i] = src[((size_t)o * K + c) * T + tap];
  }
}

struct HDgrad {
  const float* g;      // chunk-local masked gradient of the first layer's pre-activation [chunk][HID]
  const float* wd;     // [9][HID][K]: the first layer's weights, K-major over the outputs o
  float* gx;           // (B,h,w,gxs): columns c < cx; float atomics; null: skipped
  float* gx2;          // (B,h,w,gx2s): columns cx <= c < K; null: skipped
  const int* idx;
  const int* count;
  int M, begin, chunk, K, cx, gxs, gx2s, h, w;
};

// One wave = 32 list positions x 32 input channels, once per tap: D[position][c] = sum_o g[position][o] wd[tap][o][c], two o per
// MFMA, then added at the pixel the tap points to.  The accumulator's lane index is the channel: one register is two 128-byte
// segments in two pixel rows.  Whether a tap's pixel exists is decided from (b, y, x) - a neighbour outside the image, or in the
// next one, receives nothing - and only then does the linear index move.  The 16 adds of a tap go out together behind its 128
// MFMAs: an add stays counted among the outstanding memory operations for thousands of cycles and every load issued behind it
// waits for it, so adds spread through the k loop (one per 8 MFMAs, measured: 2,970 cycles per k step) stall each step, a burst
// stalls once per tap.  The operands of k step i + 1 are loaded ahead of the MFMAs of step i.
struct DgradOps {
  f32x4 a4[2];
  float bw[2][4];
};

// half 0 holds outputs 16 i .. + 3 (and + 8), half 1 the four behind them (arow / wcol carry the half's offset)
__device__ __forceinline__ void dgrad_load(DgradOps& t, const float* arow, const float* wcol, int K, int i) {
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int kb = 16 * i + 8 * v;
    t.a4[v] = *reinterpret_cast<const f32x4*>(arow + kb);
#pragma unroll
    for (int s = 0; s < 4; ++s) t.bw[v][s] = wcol[(size_t)(kb + s) * K];
  }
}

__device__ __forceinline__ void dgrad_mfma(f32x16& acc, const DgradOps& t, bool live) {
#pragma unroll
  for (int v = 0; v < 2; ++v)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? t.a4[v][s] : 0.0f, t.bw[v][s], acc, 0, 0, 0);
}

__global__ __launch_bounds__(64) void head_dgrad_kernel(const HDgrad p) {
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const int K = p.K;
  const int c = blockIdx.y * 32 + cl;
  const int cc = c < K ? c : K - 1;
  float* dst = nullptr;              // this lane's column of pixel 0 (null: nothing is added)
  int ds = 0;
  if (c < p.cx) {
    if (p.gx) { dst = p.gx + c; ds = p.gxs; }
  } else if (c < K) {
    if (p.gx2) { dst = p.gx2 + (c - p.cx); ds = p.gx2s; }
  }
  const int hw = p.h * p.w;
  for (int q0 = p.begin + blockIdx.x * GEMM_PX; q0 < end; q0 += gridDim.x * GEMM_PX) {
    // the 16 positions of this lane's accumulator registers: pixel index and the taps whose pixel lies inside the image
    int pix[16], inside[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const bool on = qq < end && dst;
      const int pv = p.idx[qq < end ? qq : end - 1];
      const int pb = pv / hw, rem = pv - pb * hw;
      const int py = rem / p.w, px = rem - py * p.w;
      int m = 0;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        m |= (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) ? 1 << tap : 0;
      }
      pix[r] = pv;
      inside[r] = on ? m : 0;
    }
    const int q = q0 + cl;
    const bool live = q < end;
    const float* arow = p.g + (size_t)((live ? q : end - 1) - p.begin) * HID + 4 * half;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int poff = (tap / 3 - 1) * p.w + tap % 3 - 1;
      const float* wcol = p.wd + ((size_t)tap * HID + 4 * half) * K + cc;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      DgradOps even, odd;
      dgrad_load(even, arow, wcol, K, 0);
#pragma unroll 1
      for (int i = 0; i < HID / 16; i += 2) {
        dgrad_load(odd, arow, wcol, K, i + 1);
        __builtin_amdgcn_sched_barrier(0);
        dgrad_mfma(acc, even, live);
        __builtin_amdgcn_sched_barrier(0);
        dgrad_load(even, arow, wcol, K, (i + 2) & (HID / 16 - 1));     // (the last step's is not used: the address stays inside)
        __builtin_amdgcn_sched_barrier(0);
        dgrad_mfma(acc, odd, live);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (inside[r] >> tap & 1) atomicAdd(dst + (size_t)(pix[r] + poff) * ds, acc[r]);
    }
  }
}

// dst[(tap * HID + o) * K + c] = src[(o * K + c) * 9 + tap]: the raw (256, K, 3, 3) weight, K-major over o
__global__ __launch_bounds__(256) void head_wd_kernel(const float* __restrict__ src, float* __restrict__ dst, int K) {
  const int n = 9 * K * HID;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int c = i % K, to = i / K;
    const int o = to & (HID - 1), tap = to >> 8;
    dst[i] = src[((size_t)o * K + c) * 9 + tap];
  }
}

// the list of pixels where any channel of gy (NCHW) is non-zero; *count zeroed by the caller
__global__ __launch_bounds__(256) void head_compact_kernel(const float* __restrict__ gy, int M, int hw, int n_out,
                                                           int* __restrict__ idx, int* __restrict__ count) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  bool any = false;
  if (m < M) {
    const int b = m / hw, rem = m - b * hw;
    const float* g = gy + (size_t)b * n_out * hw + rem;
    for (int o = 0; o < n_out; ++o) any |= g[(size_t)o * hw] != 0.0f;
  }
  const unsigned long long bal = __ballot(any);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && bal) base = atomicAdd(count, __popcll(bal));
  base = __shfl(base, 0, 64);
  if (any) idx[base + __popcll(bal & ((1ull << lane) - 1ull))] = m;
}

struct HOut {
  const float* hmap;   // chunk-local last hidden map [chunk][HID]
  const float* wout;   // raw [n_out][HID]
  const float* bout;
  float* y;            // forward: NCHW out
  const float* gy;     // backward: NCHW
  float* g;            // backward: chunk-local [chunk][HID]
  float* gw;           // [n_out][HID], float atomics
  float* gb;           // [n_out]
  const int* idx;
  const int* count;
  int M, begin, chunk, hw, n_out;
};

__device__ __forceinline__ size_t nchw_at(int pix, int hw, int n_out) {
  const int b = pix / hw;
  return (size_t)b * n_out * hw + (pix - b * hw);
}

// y[pixel][o] = bout[o] + sum_c h[pixel][c] wout[o][c]: one thread per (list position, o)
__global__ __launch_bounds__(256) void head_out_fwd_kernel(const HOut p) {
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const long n = (long)(end - p.begin) * p.n_out;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int lr = (int)(i / p.n_out), o = (int)(i - (long)lr * p.n_out);
    const f32x4* hr = reinterpret_cast<const f32x4*>(p.hmap + (size_t)lr * HID);
    const float* wr = p.wout + (size_t)o * HID;      // (a caller's parameter: no alignment assumed)
    float acc = 0.0f;
    for (int c = 0; c < HID / 4; ++c) {
      const f32x4 a = hr[c];
      acc = fmaf(a[0], wr[4 * c], acc);
      acc = fmaf(a[1], wr[4 * c + 1], acc);
      acc = fmaf(a[2], wr[4 * c + 2], acc);
      acc = fmaf(a[3], wr[4 * c + 3], acc);
    }
    const int q = p.begin + lr;
    const int pix = p.idx ? p.idx[q] : q;
    p.y[nchw_at(pix, p.hw, p.n_out) + (size_t)o * p.hw] = acc + p.bout[o];
  }
}

// g[pixel][c] = h[pixel][c] > 0 ? sum_o gy[pixel][o] wout[o][c] : 0: one thread per (list position, c)
__global__ __launch_bounds__(256) void head_out_bwd_data_kernel(const HOut p) {
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const int c = threadIdx.x;
  for (int q = p.begin + blockIdx.x; q < end; q += gridDim.x) {
    const int pix = p.idx ? p.idx[q] : q;
    const float* gy = p.gy + nchw_at(pix, p.hw, p.n_out);
    float acc = 0.0f;
    for (int o = 0; o < p.n_out; ++o) acc = fmaf(gy[(size_t)o * p.hw], p.wout[o * HID + c], acc);
    const size_t li = (size_t)(q - p.begin) * HID + c;
    p.g[li] = p.hmap[li] > 0.0f ? acc : 0.0f;
  }
}

// gw[o][c] += sum over a slab of gy[pixel][o] h[pixel][c] (thread = c); gb[o] += sum gy[pixel][o] (thread = o)
constexpr int OUT_SLAB = 128;
__global__ __launch_bounds__(256) void head_out_bwd_weight_kernel(const HOut p) {
  const int end = list_end(p.count, p.M, p.begin, p.chunk);
  const int qb = p.begin + blockIdx.x * OUT_SLAB;
  const int qe = min(end, qb + OUT_SLAB);
  if (qb >= qe) return;
  const int c = threadIdx.x;
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = 0.0f;
  float bs = 0.0f;
  for (int q = qb; q < qe; ++q) {
    const int pix = p.idx ? p.idx[q] : q;
    const float* gy = p.gy + nchw_at(pix, p.hw, p.n_out);
    const float hv = p.hmap[(size_t)(q - p.begin) * HID + c];
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      const float gv = gy[(size_t)min(o, p.n_out - 1) * p.hw];
      acc[o] = fmaf(o < p.n_out ? gv : 0.0f, hv, acc[o]);
    }
    if (c < p.n_out) bs += gy[(size_t)c * p.hw];
  }
#pragma unroll
  for (int o = 0; o < 16; ++o)
    if (o < p.n_out) atomicAdd(p.gw + o * HID + c, acc[o]);
  if (c < p.n_out) atomicAdd(p.gb + c, bs);
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Layout {
  int chunk;
  size_t wk1, wt, count, idx, bufs, wd, total;   // byte offsets
};

int resolve_chunk(long M, int chunk_px) {
  long c = chunk_px > 0 ? chunk_px : DEFAULT_CHUNK;
  const long mr = (M + 63) / 64 * 64;
  if (c > mr) c = mr;
  return (int)c;
}

Layout layout(int B, int h, int w, int Cin, int n_hidden, int chunk_px, bool backward, bool dx = false) {
  Layout L{};
  const long M = (long)B * h * w;
  L.chunk = resolve_chunk(M, chunk_px);
  size_t at = 0;
  L.wk1 = at; at += align16((size_t)9 * Cin * HID * 4);
  L.wt = at; at += align16((size_t)n_hidden * HID * HID * 4);
  L.count = at; at += 16;
  L.idx = at; at += backward ? align16((size_t)M * 4) : 0;
  L.bufs = at; at += (size_t)(backward ? n_hidden + 3 : 2) * L.chunk * HID * 4;
  L.wd = at; at += dx ? align16((size_t)9 * Cin * HID * 4) : 0;     // (behind everything cf_head_backward lays out)
  L.total = at;
  return L;
}

// where cf_head_backward_dx leaves the sources' gradient
struct DxOut {
  float* gx;
  float* gx2;
  int gxs, gx2s;
};

int head_check(const cf_head_train_args* a, const char* who, bool backward, const DxOut* dx = nullptr) {
  CF_REQUIRE(a != nullptr, "%s: null args", who);
  CF_REQUIRE(a->B > 0 && a->h > 0 && a->w > 0, "%s: bad geometry", who);
  CF_REQUIRE(a->n_hidden >= 0 && a->n_hidden <= CF_HEAD_TRAIN_MAX_HIDDEN, "%s: n_hidden=%d outside 0..%d", who, a->n_hidden,
             CF_HEAD_TRAIN_MAX_HIDDEN);
  CF_REQUIRE(a->n_out >= 1 && a->n_out <= 16, "%s: n_out=%d outside 1..16", who, a->n_out);
  CF_REQUIRE(a->hidden == HID, "%s: hidden width %d: only 256 is implemented", who, a->hidden);
  CF_REQUIRE(a->x && a->c_x >= 1 && a->x_stride >= a->c_x, "%s: x / c_x / x_stride", who);
  CF_REQUIRE(a->x2 ? (a->c_x2 >= 1 && a->x2_stride >= a->c_x2) : a->c_x2 == 0, "%s: x2 / c_x2 / x2_stride", who);
  CF_REQUIRE(a->c_x + a->c_x2 <= 512, "%s: Cin=%d above 512", who, a->c_x + a->c_x2);
  const long M = (long)a->B * a->h * a->w;
  CF_REQUIRE(M * (a->x_stride > HID ? a->x_stride : HID) < (1L << 31) && M * 16 < (1L << 31), "%s: tensor too large", who);
  if (dx) {
    CF_REQUIRE(dx->gx || dx->gx2, "%s: gx and gx2 are both null (cf_head_backward is the call without a source gradient)", who);
    CF_REQUIRE(!dx->gx || dx->gxs >= a->c_x, "%s: gx_stride=%d below c_x=%d", who, dx->gxs, a->c_x);
    CF_REQUIRE(!dx->gx2 || a->x2, "%s: gx2 without x2", who);
    CF_REQUIRE(!dx->gx2 || dx->gx2s >= a->c_x2, "%s: gx2_stride=%d below c_x2=%d", who, dx->gx2s, a->c_x2);
    CF_REQUIRE(!dx->gx || M * dx->gxs < (1L << 31), "%s: gx too large", who);
    CF_REQUIRE(!dx->gx2 || M * dx->gx2s < (1L << 31), "%s: gx2 too large", who);
  }
  CF_REQUIRE(a->chunk_px >= 0 && a->chunk_px % 64 == 0, "%s: chunk_px=%d must be a multiple of 64 (0: the default)", who, a->chunk_px);
  for (int l = 0; l < a->n_hidden + 2; ++l) {
    CF_REQUIRE(a->weight[l] && a->bias[l], "%s: null weight / bias of layer %d", who, l);
    if (backward) CF_REQUIRE(a->gw[l] && a->gb[l], "%s: null gw / gb of layer %d", who, l);
  }
  CF_REQUIRE(backward ? a->gy != nullptr : a->y != nullptr, "%s: null %s", who, backward ? "gy" : "y");
  const Layout L = layout(a->B, a->h, a->w, a->c_x + a->c_x2, a->n_hidden, a->chunk_px, backward, dx != nullptr);
  CF_REQUIRE(a->workspace && a->workspace_bytes >= L.total, "%s: workspace of %zu bytes is smaller than the %zu needed", who,
             a->workspace_bytes, L.total);
  CF_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  return CF_OK;
}

HeadSrc head_src(const cf_head_train_args* a) {
  HeadSrc s{};
  s.x = a->x; s.x2 = a->x2; s.xs = a->x_stride; s.cx = a->c_x; s.x2s = a->x2_stride; s.cx2 = a->c_x2;
  s.h = a->h; s.w = a->w;
  return s;
}

unsigned blocks_for(long n, long cap) {
  long b = (n + 255) / 256;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

// the K-major copies of the first and the hidden layers' weights
void launch_wk(const cf_head_train_args* a, const Layout& L, hipStream_t st) {
  char* ws = static_cast<char*>(a->workspace);
  const int Cin = a->c_x + a->c_x2;
  hipLaunchKernelGGL(head_wk_kernel, dim3(blocks_for(9L * Cin * HID, 1024)), dim3(256), 0, st, a->weight[0],
                     reinterpret_cast<float*>(ws + L.wk1), Cin, 9);
  for (int l = 0; l < a->n_hidden; ++l)
    hipLaunchKernelGGL(head_wk_kernel, dim3(blocks_for((long)HID * HID, 1024)), dim3(256), 0, st, a->weight[1 + l],
                       reinterpret_cast<float*>(ws + L.wt) + (size_t)l * HID * HID, HID, 1);
}

// hidden maps 0 .. n_hidden of one chunk into bufs[0 .. n_hidden] (keep_all) or ping-pong in bufs[0 / 1] -> the last map
float* launch_hidden(const cf_head_train_args* a, const Layout& L, float* const* bufs, bool keep_all, const int* idx, const int* count,
                     int begin, hipStream_t st) {
  char* ws = static_cast<char*>(a->workspace);
  const long M = (long)a->B * a->h * a->w;
  const int tiles = (L.chunk + GEMM_PX - 1) / GEMM_PX;
  const dim3 grid((unsigned)(tiles < 4096 ? tiles : 4096), HID / (32 * GEMM_NT));
  HGemm k{};
  k.s = head_src(a);
  k.wk = reinterpret_cast<const float*>(ws + L.wk1);
  k.bias = a->bias[0];
  k.out = bufs[0];
  k.idx = idx; k.count = count; k.M = (int)M; k.begin = begin; k.chunk = L.chunk; k.K = a->c_x + a->c_x2; k.mode = 0;
  k.kvec = ((reinterpret_cast<uintptr_t>(a->x) & 15) == 0 && a->x_stride % 4 == 0) ? a->c_x / 16 * 16 : 0;
  hipLaunchKernelGGL(head_gemm_kernel<9>, grid, dim3(64), 0, st, k);
  float* cur = bufs[0];
  for (int l = 0; l < a->n_hidden; ++l) {
    float* nxt = keep_all ? bufs[l + 1] : bufs[(l + 1) & 1];
    HGemm g{};
    g.s = k.s;
    g.a = cur;
    g.wk = reinterpret_cast<const float*>(ws + L.wt) + (size_t)l * HID * HID;
    g.bias = a->bias[1 + l];
    g.out = nxt;
    g.idx = idx; g.count = count; g.M = (int)M; g.begin = begin; g.chunk = L.chunk; g.K = HID; g.mode = 0; g.kvec = HID;
    hipLaunchKernelGGL(head_gemm_kernel<1>, grid, dim3(64), 0, st, g);
    cur = nxt;
  }
  return cur;
}

}  // namespace

extern "C" size_t cf_head_train_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px) {
  if (B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || n_hidden < 0 || chunk_px < 0) return 0;
  return layout(B, h, w, Cin, n_hidden, chunk_px, false).total;
}

extern "C" size_t cf_head_bwd_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px) {
  if (B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || n_hidden < 0 || chunk_px < 0) return 0;
  return layout(B, h, w, Cin, n_hidden, chunk_px, true).total;
}

extern "C" size_t cf_head_bwd_dx_workspace_bytes(int B, int h, int w, int Cin, int n_hidden, int chunk_px) {
  if (B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || n_hidden < 0 || chunk_px < 0) return 0;
  return layout(B, h, w, Cin, n_hidden, chunk_px, true, true).total;
}

extern "C" int cf_head_bwd_chunk_px(int B, int h, int w, int chunk_px) {
  if (B <= 0 || h <= 0 || w <= 0 || chunk_px < 0) return 0;
  return resolve_chunk((long)B * h * w, chunk_px);
}

extern "C" int cf_head_train_forward(const cf_head_train_args* a, void* stream) {
  if (int e = head_check(a, "cf_head_train_forward", false)) return e;
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout(a->B, a->h, a->w, a->c_x + a->c_x2, a->n_hidden, a->chunk_px, false);
  char* ws = static_cast<char*>(a->workspace);
  float* base = reinterpret_cast<float*>(ws + L.bufs);
  float* bufs[2] = {base, base + (size_t)L.chunk * HID};
  const long M = (long)a->B * a->h * a->w;
  launch_wk(a, L, st);
  for (long begin = 0; begin < M; begin += L.chunk) {
    float* last = launch_hidden(a, L, bufs, false, nullptr, nullptr, (int)begin, st);
    HOut o{};
    o.hmap = last; o.wout = a->weight[a->n_hidden + 1]; o.bout = a->bias[a->n_hidden + 1]; o.y = a->y;
    o.M = (int)M; o.begin = (int)begin; o.chunk = L.chunk; o.hw = a->h * a->w; o.n_out = a->n_out;
    hipLaunchKernelGGL(head_out_fwd_kernel, dim3(blocks_for((long)L.chunk * a->n_out, 4096)), dim3(256), 0, st, o);
  }
  return cf_check_launch("cf_head_train_forward");
}

namespace {

// cf_head_backward (dx null) and cf_head_backward_dx: the same launches, and behind each chunk's the scatter of dX
int head_backward(const cf_head_train_args* a, const char* who, const DxOut* dx, void* stream) {
  if (int e = head_check(a, who, true, dx)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int Cin = a->c_x + a->c_x2, nh = a->n_hidden;
  const Layout L = layout(a->B, a->h, a->w, Cin, nh, a->chunk_px, true, dx != nullptr);
  char* ws = static_cast<char*>(a->workspace);
  int* count = reinterpret_cast<int*>(ws + L.count);
  int* idx = reinterpret_cast<int*>(ws + L.idx);
  float* base = reinterpret_cast<float*>(ws + L.bufs);
  float* bufs[CF_HEAD_TRAIN_MAX_HIDDEN + 3];
  for (int i = 0; i < nh + 3; ++i) bufs[i] = base + (size_t)i * L.chunk * HID;
  const long M = (long)a->B * a->h * a->w;
  const int hw = a->h * a->w;
  if (hipMemsetAsync(count, 0, 16, st) != hipSuccess) return cf_check_launch(who);
  (void)hipMemsetAsync(a->gw[0], 0, (size_t)HID * Cin * 9 * 4, st);
  for (int l = 1; l <= nh; ++l) (void)hipMemsetAsync(a->gw[l], 0, (size_t)HID * HID * 4, st);
  (void)hipMemsetAsync(a->gw[nh + 1], 0, (size_t)a->n_out * HID * 4, st);
  for (int l = 0; l <= nh; ++l) (void)hipMemsetAsync(a->gb[l], 0, (size_t)HID * 4, st);
  (void)hipMemsetAsync(a->gb[nh + 1], 0, (size_t)a->n_out * 4, st);
  hipLaunchKernelGGL(head_compact_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, a->gy, (int)M, hw, a->n_out, idx, count);
  launch_wk(a, L, st);
  if (dx) {
    // zeroed once, padding channels included: neighbouring pixels of different chunks add into the same rows
    if (dx->gx) (void)hipMemsetAsync(dx->gx, 0, (size_t)M * dx->gxs * 4, st);
    if (dx->gx2) (void)hipMemsetAsync(dx->gx2, 0, (size_t)M * dx->gx2s * 4, st);
    hipLaunchKernelGGL(head_wd_kernel, dim3(blocks_for(9L * Cin * HID, 1024)), dim3(256), 0, st, a->weight[0],
                       reinterpret_cast<float*>(ws + L.wd), Cin);
  }
  const int slabs = (L.chunk + SLAB_PX - 1) / SLAB_PX;
  const int tiles = (L.chunk + GEMM_PX - 1) / GEMM_PX;
  for (long begin = 0; begin < M; begin += L.chunk) {
    float* last = launch_hidden(a, L, bufs, true, idx, count, (int)begin, st);
    float* g = bufs[nh + 1];
    float* g2 = bufs[nh + 2];
    HOut o{};
    o.hmap = last; o.wout = a->weight[nh + 1]; o.gy = a->gy; o.g = g; o.gw = a->gw[nh + 1]; o.gb = a->gb[nh + 1];
    o.idx = idx; o.count = count; o.M = (int)M; o.begin = (int)begin; o.chunk = L.chunk; o.hw = hw; o.n_out = a->n_out;
    hipLaunchKernelGGL(head_out_bwd_weight_kernel, dim3((unsigned)((L.chunk + OUT_SLAB - 1) / OUT_SLAB)), dim3(256), 0, st, o);
    hipLaunchKernelGGL(head_out_bwd_data_kernel, dim3((unsigned)(L.chunk < 4096 ? L.chunk : 4096)), dim3(256), 0, st, o);
    for (int l = nh; l >= 1; --l) {
      HWgrad wg{};
      wg.s = head_src(a);
      wg.a = bufs[l - 1]; wg.g = g; wg.gw = a->gw[l]; wg.gb = a->gb[l];
      wg.idx = idx; wg.count = count; wg.M = (int)M; wg.begin = (int)begin; wg.chunk = L.chunk; wg.K = HID;
      wg.ostride = HID; wg.cstride = 1;
      hipLaunchKernelGGL(head_wgrad_kernel<1>, dim3((unsigned)slabs, HID / 32, 2), dim3(64), 0, st, wg);
      HGemm c{};
      c.s = wg.s;
      c.a = g; c.wk = a->weight[l]; c.mask = bufs[l - 1]; c.out = g2;
      c.idx = idx; c.count = count; c.M = (int)M; c.begin = (int)begin; c.chunk = L.chunk; c.K = HID; c.mode = 1; c.kvec = HID;
      hipLaunchKernelGGL(head_gemm_kernel<1>, dim3((unsigned)(tiles < 4096 ? tiles : 4096), HID / (32 * GEMM_NT)), dim3(64), 0, st, c);
      float* t = g; g = g2; g2 = t;
    }
    HWgrad w1{};
    w1.s = head_src(a);
    w1.g = g; w1.gw = a->gw[0]; w1.gb = a->gb[0];
    w1.idx = idx; w1.count = count; w1.M = (int)M; w1.begin = (int)begin; w1.chunk = L.chunk; w1.K = Cin;
    w1.ostride = Cin * 9; w1.cstride = 9;
    hipLaunchKernelGGL(head_wgrad_kernel<9>, dim3((unsigned)slabs, (unsigned)(9 * ((Cin + 31) / 32)), 2), dim3(64), 0, st, w1);
    if (dx) {
      HDgrad d{};
      d.g = g; d.wd = reinterpret_cast<const float*>(ws + L.wd); d.gx = dx->gx; d.gx2 = dx->gx2;
      d.idx = idx; d.count = count; d.M = (int)M; d.begin = (int)begin; d.chunk = L.chunk; d.K = Cin; d.cx = a->c_x;
      d.gxs = dx->gxs; d.gx2s = dx->gx2s; d.h = a->h; d.w = a->w;
      hipLaunchKernelGGL(head_dgrad_kernel, dim3((unsigned)(tiles < 4096 ? tiles : 4096), (unsigned)((Cin + 31) / 32)), dim3(64), 0, st, d);
    }
  }
  return cf_check_launch(who);
}

}  // namespace

extern "C" int cf_head_backward(const cf_head_train_args* a, void* stream) {
  return head_backward(a, "cf_head_backward", nullptr, stream);
}

extern "C" int cf_head_backward_dx(const cf_head_train_args* a, float* gx, int gx_stride, float* gx2, int gx2_stride, void* stream) {
  const DxOut dx{gx, gx2, gx_stride, gx2_stride};
  return head_backward(a, "cf_head_backward_dx", &dx, stream);
}
