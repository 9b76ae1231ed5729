// Implicit-GEMM convolution with fp32 STORAGE and split-fp16 COMPUTE ("f16x3") on the gfx950 f16 MFMA
// pipe - the fast path for the backbone / offset convolutions, whose rounding must stay at fp32 level
// because the DCN neck amplifies it ~100x (DESIGN.md §4 Numerics).
//
// Numerics.  An fp32 operand x (times a power-of-two scale that keeps its low part out of the fp16
// subnormal range) is split into hi = rne_f16(x), lo = rne_f16(x - hi): hi + lo carries ~22-24
// significant bits.  A product is  a_hi*b_hi + (a_lo*b_hi + a_hi*b_lo)  - three
// v_mfma_f32_32x32x16_f16 per 16-deep k-step (the dropped a_lo*b_lo term is < 2^-22 relative).  Each
// MFMA sums its 16 products before ONE fp32 rounding into the accumulator, so the rounding chain is
// K/16 long instead of K (fp32 MFMA 32x32x2: K/2); the two small cross terms go to their own
// accumulator so they do not add rounding steps to the main sum.  CPU emulation and the measured
// end-to-end error put this at the level of the two-level fp32 path (tools/stage_error.py).
// Scales: weights are pre-multiplied by 2^s per layer (host, max|w| -> ~2^14), activations by 2^4 at
// staging; the epilogue multiplies by 2^-(s+4) - all exact.  Activations must satisfy |x| < 4094
// (fp16 range after the 2^4 scale); they are clamped there, which only matters for absurd inputs.
//
// Structure (same SWAPPED orientation as cf_heads.hip): MFMA A-operand = weights, pre-packed on the
// host in fragment order and read straight from L2 (2 k-steps ahead in registers, no LDS, no
// barrier); B-operand = pixels: the fp32 NHWC activations are gathered per 8-channel slot, split to
// fp16 hi/lo on the fly and staged through a double-buffered LDS tile [64*WP px][32 k] - one barrier
// per 32-deep chunk.  Workgroup = 4 waves as WC (channel groups) x WP (pixel groups); a wave owns
// RT*32 output channels x 64 pixels.  Accumulators have pixels on lanes and 4 consecutive channels
// per register group, so the fp32 NHWC store is one 16-byte write per lane and group.
#include "cf_f16x3.h"
#include "cf_mx.h"

namespace {

struct ConvF {
  const float* src[CF_MAX_SRC];
  int src_c[CF_MAX_SRC];
  const unsigned char* weight;  // [N_pad/32][K_pad/16][2][64][8 f16]
  const cf_slot* slots;         // 8-channel slots, 4 per chunk
  const float* bias;
  const float* residual;
  float* out;
  int H, W, Ho, Wo, stride, n_chunks, res_stride, out_stride, act, M, N, HoWo, n_rt;
  float out_scale;
  float in_scale;               // activation pre-scale (power of two)
};

// DB: double-buffered pixel tile (one barrier per chunk).  The 256-pixel tile of the 64-channel
// layers (WP = 4) is single-buffered (two barriers per chunk) so two workgroups still fit a CU.
template <int WC, int WP, int RT, bool DB>
__global__ __launch_bounds__(256, 2) void conv_f16x3_kernel(ConvF p) {
  static_assert(WC * WP == 4, "4 waves per workgroup");
  constexpr int PXB = 64 * WP;             // pixels per workgroup
  constexpr int PLANE = PXB * FROWB;       // bytes per plane of one chunk buffer
  constexpr int BUF = 2 * PLANE;
  constexpr int EROW = RT * 128 + 16;      // epilogue: a wave's 32 pixels x 32*RT channels, transposed through LDS
  constexpr int SMEM = (DB ? 2 : 1) * BUF > 4 * 32 * EROW ? (DB ? 2 : 1) * BUF : 4 * 32 * EROW;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
  extern __shared__ __attribute__((aligned(16))) cf_slot lds_slots[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: scalar tile / weight addressing)
  const int li = lane & 31, h = lane >> 5;
  const int wc = wave / WP, wp = wave % WP;
  const int m0 = cf_xcd_remap(blockIdx.x, gridDim.x) * PXB;   // consecutive pixel tiles share an XCD (L2)
  const int rt0 = (blockIdx.y * WC + wc) * RT;          // first 32-row tile of this wave
  const bool w_ok = rt0 < p.n_rt;                       // (RT divides the padded tile count)
  const int n_ks = p.n_chunks * 2;
  for (int i = tid; i < p.n_chunks * 4; i += 256) lds_slots[i] = p.slots[i];

  // staging role: WP (pixel, 8-channel unit) pairs per thread
  int y0[WP], x0[WP], boff[WP];
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int px = (tid + 256 * i) >> 2;
    const int m = m0 + px;
    if (m < p.M) {
      const int b = m / p.HoWo, rem = m - b * p.HoWo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      y0[i] = ho * p.stride;
      x0[i] = wo * p.stride;
      boff[i] = b * p.H * p.W;
    } else {
      y0[i] = -(1 << 28);
      x0[i] = 0;
      boff[i] = 0;
    }
  }
  __syncthreads();

  f32x4 raw[WP][2];
  auto load_b = [&](int c) {
    const int src = __builtin_amdgcn_readfirstlane(lds_slots[c * 4].src);
    const float* sp = src == 1 ? p.src[1] : src == 2 ? p.src[2] : src == 3 ? p.src[3] : p.src[0];
    const int sc = src == 1 ? p.src_c[1] : src == 2 ? p.src_c[2] : src == 3 ? p.src_c[3] : p.src_c[0];
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const cf_slot s = lds_slots[c * 4 + (tid & 3)];
      const int y = y0[i] + s.dy, x = x0[i] + s.dx;
      const bool ok = (s.c_off >= 0) && ((unsigned)y < (unsigned)p.H) && ((unsigned)x < (unsigned)p.W);
      raw[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      raw[i][1] = raw[i][0];
      if (ok) {
        const float* a = sp + (size_t)(boff[i] + y * p.W + x) * sc + s.c_off;
        raw[i][0] = *reinterpret_cast<const f32x4*>(a);
        raw[i][1] = *reinterpret_cast<const f32x4*>(a + 4);
      }
    }
  };
  auto store_b = [&](unsigned char* buf) {
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int pr = tid + 256 * i;
      u32x4 hi, lo;
      split8(raw[i][0], raw[i][1], hi, lo, p.in_scale);
      unsigned char* o = buf + (pr >> 2) * FROWB + (pr & 3) * 16;
      *reinterpret_cast<u32x4*>(o) = hi;
      *reinterpret_cast<u32x4*>(o + PLANE) = lo;
    }
  };

  f32x16 accm[RT][2], accs[RT][2];   // main (hi*hi) and small (lo*hi + hi*lo) sums
#pragma unroll
  for (int a = 0; a < RT; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accm[a][b][r] = 0.0f;
        accs[a][b][r] = 0.0f;
      }

  f16x8 wh[2][RT], wl[2][RT];        // weight fragments of k-steps (2n) and (2n+1)
  auto load_w = [&](f16x8 (&dh)[RT], f16x8 (&dl)[RT], int ks) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      dh[rt] = *wfrag16(p.weight, w_ok ? rt0 + rt : 0, ks, 0, n_ks, lane);
      dl[rt] = *wfrag16(p.weight, w_ok ? rt0 + rt : 0, ks, 1, n_ks, lane);
    }
  };
  auto mma_kstep = [&](const unsigned char* buf, int s, const f16x8 (&ah)[RT], const f16x8 (&al)[RT]) {
    f16x8 xh[2], xl[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const unsigned char* row = buf + (wp * 64 + ct * 32 + li) * FROWB + s * 32 + h * 16;
      xh[ct] = *reinterpret_cast<const f16x8*>(row);
      xl[ct] = *reinterpret_cast<const f16x8*>(row + PLANE);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[rt], xh[ct], accs[rt][ct], 0, 0, 0);
        accs[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xl[ct], accs[rt][ct], 0, 0, 0);
        accm[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[rt], xh[ct], accm[rt][ct], 0, 0, 0);
      }
  };

  load_b(0);
  load_w(wh[0], wl[0], 0);
  load_w(wh[1], wl[1], 1);
  store_b(smem);
  load_b(p.n_chunks > 1 ? 1 : 0);
  __syncthreads();
  // Straight-line body (indices clamped instead of branches) so the scheduler may interleave the
  // VALU operand split of chunk c+1 with the MFMAs of chunk c (sched_group_barrier pattern below).
  const int last = p.n_chunks - 1;
  for (int c = 0; c < p.n_chunks; ++c) {
    unsigned char* cur = smem + (DB ? (c & 1) * BUF : 0);
    unsigned char* nxt = smem + (DB ? ((c + 1) & 1) * BUF : 0);
    mma_kstep(cur, 0, wh[0], wl[0]);
    load_w(wh[0], wl[0], min(2 * c + 2, n_ks - 2));
    if (!DB) {
      mma_kstep(cur, 1, wh[1], wl[1]);
      load_w(wh[1], wl[1], min(2 * c + 3, n_ks - 1));
      __syncthreads();                      // single buffer: everyone is done reading it
      store_b(nxt);
    } else {
      store_b(nxt);                         // chunk c+1 (requested one chunk ago): VALU split + 2 LDS writes
      mma_kstep(cur, 1, wh[1], wl[1]);
      load_w(wh[1], wl[1], min(2 * c + 3, n_ks - 1));
#pragma unroll
      for (int i = 0; i < 6 * RT; ++i) {    // pair every MFMA of the chunk with a few VALU / DS ops
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 4 * WP, 0);   // VALU
      }
    }
    load_b(min(c + 2, last));
    __syncthreads();
  }

  // ---- epilogue, coalesced (see cf_conv3x3_f16.hip): each wave transposes its 32 pixels x 32*RT channels through a
  // private LDS tile (free after the loop's last barrier) and stores / reads the residual as whole pixel rows
  if (w_ok) {
    constexpr int LPP = RT * 8, PPI = 64 / LPP;
    asm volatile("; cf_epilogue_begin" ::: "memory");   // marker for tools/check_isa.py (no instruction)
    unsigned char* eb = smem + wave * 32 * EROW;
    const int chunk = lane % LPP, psub = lane / LPP;
    const int n = rt0 * 32 + chunk * 4;
    f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.N) bias4[e] = p.bias[n + e];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      if (ct) cf_wave_lds_sync();            // ... and every lane has read the previous tile before it is overwritten
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (accm[rt][ct][g * 4 + e] + accs[rt][ct][g * 4 + e]) * p.out_scale;
          *reinterpret_cast<f32x4*>(eb + li * EROW + (rt * 32 + 8 * g + 4 * h) * 4) = v;
        }
      cf_wave_lds_sync();                    // the tile is complete before any lane reads another lane's part ...
#pragma unroll
      for (int it = 0; it < 32 / PPI; ++it) {
        const int ploc = it * PPI + psub;
        const size_t m = (size_t)m0 + wp * 64 + ct * 32 + ploc;
        f32x4 v = *reinterpret_cast<const f32x4*>(eb + ploc * EROW + chunk * 16) + bias4;
        if (m >= (size_t)p.M || n >= p.N) continue;
        if (n + 3 < p.N) {
          if (p.residual) v += *reinterpret_cast<const f32x4*>(p.residual + m * p.res_stride + n);
          if (p.act == CF_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
          }
          *reinterpret_cast<f32x4*>(p.out + m * p.out_stride + n) = v;
        } else {                             // last, partial group of channels: element by element
          for (int e = 0; e < 4 && n + e < p.N; ++e) {
            float x = v[e];
            if (p.residual) x += p.residual[m * p.res_stride + n + e];
            if (p.act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
            p.out[m * p.out_stride + n + e] = x;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// DCNv2 main GEMM on the same f16x3 scheme.  The B operand is the bilinear sample: per (pixel, tap)
// the sampling position and 16*sigmoid(mask) are computed once per tile into LDS; per chunk a thread
// requests the 4 corner rows (8 fp32 channels each) of its (pixel, unit) pairs one chunk ahead,
// combines them in fp32, splits to fp16 hi/lo and stages them.  The VALU work per sample (~14
// instructions) is what bounds the 64-output-channel layers, not the MFMA pipe.
// ---------------------------------------------------------------------------------------------
struct DcnF {
  const float* x;
  const float* om;
  const unsigned char* weight;
  const float* bias;
  float* out;
  int om_stride, H, W, C, n_chunks, chunks_per_tap, out_stride, act, M, N, n_rt;
  float out_scale;
  float in_scale;        // activation pre-scale (power of two), carried by the modulation factor
  float mx_scale;        // pre-scale of the mx rows (out_mx)
  unsigned* out_split;   // optional split-bf16 copy [M][2][split_stride] (as 32-bit words: 2 bf16 each)
  int split_stride;
  unsigned char* out_mx; // optional mx rows [M][272] (cf_pack_feat_mx's format; N = 64, one 32-channel row tile per wave)
  float* partial;        // K split (gridDim.z > 1): raw partial sums [z][M][n_rt * 32], reduced by dcn_reduce_kernel
  int direct_epilogue;   // always 0: no kernel reads it, it only keeps its slot in the argument block
  int mask_activated;    // offmask channels 18..26 are modulation factors already (no sigmoid here)
};

// CT = 32-pixel column tiles per wave: 2 (64 pixels per wave), or 1 - half-size pixel tiles: half the accumulators and half the corner
// registers per thread, half the LDS: three workgroups per CU instead of two where a wave's chain has nothing to hide behind.
// GROUPED form (cf_dcn_v2_f16x3_grouped): n_groups layers of one geometry as one grid of n_groups x tiles workgroups.  Workgroup
// b serves group b / n_tiles as tile b % n_tiles of that group: m0 and every test against M stay group-local; the group picks
// x, weight, bias and the scales, and rows [g M, (g + 1) M) of om / out / every z plane of partial.
constexpr int CF_GROUPS = 4;
struct DcnG {
  int n_tiles;                                  // workgroups (gridDim.x) per group
  int M_all;                                    // n_groups * M: rows of one z plane of partial
  const float* x[CF_GROUPS];
  const unsigned char* weight[CF_GROUPS];
  const float* bias[CF_GROUPS];
  float in_scale[CF_GROUPS], out_scale[CF_GROUPS];
};

#define CF_DCN_GROUPED 0
#include "cf_dcn_f16_kernel.h"   // dcn_f16x3_kernel
#undef CF_DCN_GROUPED
#define CF_DCN_GROUPED 1
#include "cf_dcn_f16_kernel.h"   // dcn_f16x3_kernel_grouped
#undef CF_DCN_GROUPED

// K-split reduction: out = act((sum_z partial[z]) * out_scale + bias), partials added in z order
__global__ __launch_bounds__(256) void dcn_reduce_kernel(const float* __restrict__ partial, int ks, long MN4, int ns4,
                                                         int N, const float* __restrict__ bias, float out_scale,
                                                         int act, float* __restrict__ out, int out_stride) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (long)gridDim.x * 256) {
    const long m = i / ns4;
    const int n = (int)(i - m * ns4) * 4;
    if (n >= N) continue;
    f32x4 v = reinterpret_cast<const f32x4*>(partial)[i];
    for (int z = 1; z < ks; ++z) v += reinterpret_cast<const f32x4*>(partial)[(size_t)z * MN4 + i];
    v = v * out_scale;
    for (int e = 0; e < 4 && n + e < N; ++e) {
      float x = v[e] + bias[n + e];
      if (act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
      out[(size_t)m * out_stride + n + e] = x;
    }
  }
}

// ... over the rows of every group of a grouped launch: row m belongs to group m / M, which picks the bias and the scale; the
// sum over z is the one above
struct DcnRG {
  const float* bias[CF_GROUPS];
  float out_scale[CF_GROUPS];
};
__global__ __launch_bounds__(256) void dcn_reduce_grouped_kernel(const float* __restrict__ partial, int ks, long MN4, int ns4,
                                                                 int N, int M, DcnRG g, int act, float* __restrict__ out,
                                                                 int out_stride) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (long)gridDim.x * 256) {
    const long m = i / ns4;
    const int n = (int)(i - m * ns4) * 4;
    if (n >= N) continue;
    const int grp = (int)(m / M);
    // (a select chain, not an index: the group differs between lanes)
    const float* bias = grp == 0 ? g.bias[0] : grp == 1 ? g.bias[1] : grp == 2 ? g.bias[2] : g.bias[3];
    const float out_scale = grp == 0 ? g.out_scale[0] : grp == 1 ? g.out_scale[1] : grp == 2 ? g.out_scale[2] : g.out_scale[3];
    f32x4 v = reinterpret_cast<const f32x4*>(partial)[i];
    for (int z = 1; z < ks; ++z) v += reinterpret_cast<const f32x4*>(partial)[(size_t)z * MN4 + i];
    v = v * out_scale;
    for (int e = 0; e < 4 && n + e < N; ++e) {
      float x = v[e] + bias[n + e];
      if (act == CF_ACT_RELU) x = fmaxf(x, 0.0f);
      out[(size_t)m * out_stride + n + e] = x;
    }
  }
}

// number of K parts of a DCN launch on an H x W map (per-image geometry only)
int dcn_k_split(int H, int W, int n_chunks, int n_pad) {
  const long hw = (long)H * W;
  int ks = hw <= 512 ? 4 : (hw <= 2048 && n_pad <= 128) ? 2 : 1;   // (256 outputs at 28x50: the reduction pass costs what the split saves)
  while (ks > 1 && n_chunks < 4 * ks) ks >>= 1;
  return ks;
}

template <typename K, typename... A>
void launch_f16(K kernel, dim3 grid, size_t dyn, hipStream_t st, const A&... args) {
  static CfLdsLimit lds_limit;  // one per template instantiation
  lds_limit.ensure(kernel, dyn, 16384);
  hipLaunchKernelGGL(kernel, grid, dim3(256), dyn, st, args...);
}

// The tile form of a DCN launch: dcn_f16x3_kernel<WC, WP, RT, COAL, CT> (n_groups > 1: dcn_f16x3_kernel_grouped) on the grid
// (n_groups x tiles, grid_y, ks).
struct DcnForm {
  int WC, WP, RT;
  bool COAL;
  int CT;
  unsigned tiles, grid_y, ks;
};

// The one place that form is chosen (cf_dcn_v2_f16x3_form reports it, cf_dcn_v2_f16x3 and _grouped run it): M pixels per
// group, ks from dcn_k_split, G groups - the small-grid rule sees the whole grid, it changes no sum.
DcnForm dcn_pick(long M, int N, int N_pad, unsigned ks, long G) {
  const bool coal = (N & 3) == 0;   // whole-row epilogue through LDS
  const unsigned tiles64 = (unsigned)((M + 63) / 64), tiles128 = (unsigned)((M + 127) / 128);
  // SMALL GRIDS (small batches): 64 output channels on 64-pixel tiles (the 128-channel configuration with two of its
  // four channel-group waves idle in the MFMAs, all four staging) while that launch still fits the chip in one round:
  // 128 -> 64 at 56x100, bs=1: 30.4 vs 43.4 us, bs=2: 31.6 vs 45.0 us; at 350 workgroups the gain is gone.  Same K order,
  // same K split: bit-identical, so the choice may depend on the batch size (as in cf_conv3x3_f16x3).
  if (N_pad <= 64 && (M + 63) / 64 * (long)ks * G <= 256) return {4, 1, 1, coal, 2, tiles64, 1u, ks};
  // 64 channels: 2 x 32-channel wave rows, 2 x 64 pixels - or, with the whole-row epilogue,
  // half-size pixel tiles (32 pixels per wave: 114 registers, 39 KB of LDS - four workgroups per CU instead of two): the parts
  // of this kernel add up instead of overlapping (docs/experiments/r5_dcn_attribution.md), so a third wave per SIMD pays
  // wherever the grid is not many rounds deep - 8 x 64 -> 64 at 112 x 200: 116.5 vs 123.5 us, 8 x 128 -> 64 at 56 x 100: 61.1 vs
  // 72.6 us, 16 x 64 -> 64 at 112 x 200: equal; step 7.75 vs 7.80 ms.  Same K order: bit-identical.
  if (N_pad <= 64) return {2, 2, 1, coal, coal ? 1 : 2, coal ? tiles64 : tiles128, (unsigned)((N_pad + 63) / 64), ks};
  // 128 channels: 4 x 32-channel wave rows, 64 pixels
  if (N_pad <= 128) return {4, 1, 1, coal, 2, tiles64, (unsigned)((N_pad + 127) / 128), ks};
  return {4, 1, 2, coal, 2, tiles64, (unsigned)((N_pad + 255) / 256), ks};
}

// The instantiated forms: X(WC, WP, RT, COAL, CT, has a grouped instantiation)
#define CF_DCN_TILES(X)      \
  X(4, 1, 1, true, 2, true)  \
  X(4, 1, 1, false, 2, false) \
  X(2, 2, 1, true, 1, true)  \
  X(2, 2, 1, false, 2, false) \
  X(4, 1, 2, true, 2, false) \
  X(4, 1, 2, false, 2, false)

// launches f if it is this instantiation: on grid (tiles, grid_y, ks), or (g != nullptr) the grouped form on (n_groups x tiles, grid_y, ks)
template <int WC, int WP, int RT, bool COAL, int CT, bool HAS_GRP>
bool dcn_launch_if(const DcnForm& f, const DcnF& k, DcnG* g, int n_groups, hipStream_t st) {
  if (f.WC != WC || f.WP != WP || f.RT != RT || f.COAL != COAL || f.CT != CT || (g && !HAS_GRP)) return false;
  if (!g) launch_f16(dcn_f16x3_kernel<WC, WP, RT, COAL, CT>, dim3(f.tiles, f.grid_y, f.ks), 0, st, k);
  if constexpr (HAS_GRP) {
    if (g) {
      g->n_tiles = (int)f.tiles;
      launch_f16(dcn_f16x3_kernel_grouped<WC, WP, RT, COAL, CT>, dim3(f.tiles * (unsigned)n_groups, f.grid_y, f.ks), 0, st, k, *g);
    }
  }
  return true;
}

}  // namespace

extern "C" int cf_conv2d_f16x3(const cf_conv_args* a, void* stream) {
  CF_REQUIRE(a != nullptr, "cf_conv2d_f16x3: null args");
  CF_REQUIRE(a->n_src >= 1 && a->n_src <= CF_MAX_SRC, "cf_conv2d_f16x3: n_src=%d", a->n_src);
  CF_REQUIRE(a->K_pad > 0 && a->K_pad % 32 == 0, "cf_conv2d_f16x3: K_pad=%d not a multiple of 32", a->K_pad);
  CF_REQUIRE(a->N > 0 && a->N_pad >= a->N && a->N_pad % 32 == 0, "cf_conv2d_f16x3: N=%d N_pad=%d", a->N, a->N_pad);
  CF_REQUIRE(a->N_pad == 32 || a->N_pad % 64 == 0, "cf_conv2d_f16x3: N_pad=%d must be 32 or a multiple of 64", a->N_pad);
  CF_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->Ho > 0 && a->Wo > 0 && a->stride > 0, "cf_conv2d_f16x3: bad geometry");
  CF_REQUIRE(a->weight && a->slots && a->bias && a->out, "cf_conv2d_f16x3: null buffer");
  CF_REQUIRE(a->out_layout == CF_LAYOUT_NHWC && a->out_stride >= a->N && a->out_stride % 4 == 0,
             "cf_conv2d_f16x3: output must be fp32 NHWC with a stride that is a multiple of 4");
  CF_REQUIRE(a->act == CF_ACT_NONE || a->act == CF_ACT_RELU, "cf_conv2d_f16x3: act=%d unsupported", a->act);
  CF_REQUIRE(a->out_scale > 0.0f, "cf_conv2d_f16x3: out_scale must be the 2^-(s+4) the weights were packed with");
  CF_REQUIRE(!a->residual || a->res_stride % 4 == 0, "cf_conv2d_f16x3: residual stride must be a multiple of 4");
  for (int i = 0; i < a->n_src; ++i)
    CF_REQUIRE(a->src[i] && a->src_c[i] > 0 && a->src_c[i] % 8 == 0, "cf_conv2d_f16x3: source %d invalid", i);
  const long M = (long)a->B * a->Ho * a->Wo;
  CF_REQUIRE((long)a->B * a->H * a->W < (1L << 30) && M < (1L << 31), "cf_conv2d_f16x3: tensor too large");
  ConvF k{};
  for (int i = 0; i < CF_MAX_SRC; ++i) {
    k.src[i] = i < a->n_src ? a->src[i] : nullptr;
    k.src_c[i] = i < a->n_src ? a->src_c[i] : 0;
  }
  k.weight = reinterpret_cast<const unsigned char*>(a->weight);
  k.slots = a->slots;
  k.bias = a->bias;
  k.residual = a->residual;
  k.out = a->out;
  k.H = a->H; k.W = a->W; k.Ho = a->Ho; k.Wo = a->Wo; k.stride = a->stride;
  k.n_chunks = a->K_pad / 32;
  k.res_stride = a->res_stride; k.out_stride = a->out_stride; k.act = a->act;
  k.M = (int)M; k.N = a->N; k.HoWo = a->Ho * a->Wo;
  k.n_rt = a->N_pad / 32;
  k.out_scale = a->out_scale;
  k.in_scale = cf_resolve_in_scale(a->in_scale);
  CF_REQUIRE(k.in_scale > 0.0f, "cf_conv2d_f16x3: in_scale must be 0 (= 16) or a power of two");
  const size_t dyn = (size_t)k.n_chunks * 4 * sizeof(cf_slot);
  hipStream_t st = (hipStream_t)stream;
  if (a->N_pad == 32) {
    launch_f16(conv_f16x3_kernel<1, 4, 1, false>, dim3((unsigned)((M + 255) / 256), 1), dyn, st, k);
  } else if (a->N_pad == 64) {
    launch_f16(conv_f16x3_kernel<1, 4, 2, false>, dim3((unsigned)((M + 255) / 256), 1), dyn, st, k);
  } else if (a->N_pad == 128) {
    launch_f16(conv_f16x3_kernel<2, 2, 2, true>, dim3((unsigned)((M + 127) / 128), 1), dyn, st, k);
  } else {
    launch_f16(conv_f16x3_kernel<4, 1, 2, true>, dim3((unsigned)((M + 63) / 64), (unsigned)((a->N_pad + 255) / 256)), dyn, st, k);
  }
  return cf_check_launch("cf_conv2d_f16x3");
}

// gs == nullptr: the launch of cf_dcn_v2_f16x3.  Otherwise a == gs[0] and the n_groups (>= 2) validated blocks of
// cf_dcn_v2_f16x3_grouped: the same code picks the K split and the tile form (the small-grid rule sees the whole grid - it
// changes no sum), the grid is n_groups times as wide in x, and ONE reduction runs over every group's rows.
// report != nullptr (cf_dcn_v2_f16x3_form): validate and pick as the launch does, write the answer, touch no runtime.
static int dcn_f16x3_impl(const cf_dcn_args* a, const cf_dcn_args* const* gs, int n_groups, void* stream, int32_t* report = nullptr) {
  CF_REQUIRE(a != nullptr, "cf_dcn_v2_f16x3: null args");
  CF_REQUIRE(a->C > 0 && a->C % 32 == 0, "cf_dcn_v2_f16x3: C=%d not a multiple of 32", a->C);
  CF_REQUIRE(a->N > 0 && a->N_pad >= a->N && a->N_pad % 32 == 0, "cf_dcn_v2_f16x3: N=%d N_pad=%d", a->N, a->N_pad);
  CF_REQUIRE(a->N_pad <= 128 || a->N_pad % 64 == 0, "cf_dcn_v2_f16x3: N_pad=%d above 128 must be a multiple of 64 (two row tiles per wave)", a->N_pad);
  CF_REQUIRE(a->om_stride >= 27, "cf_dcn_v2_f16x3: om_stride=%d < 27", a->om_stride);
  CF_REQUIRE(a->x && a->offmask && a->weight && a->bias && a->out, "cf_dcn_v2_f16x3: null buffer");
  CF_REQUIRE(a->out_stride >= a->N && a->out_stride % 4 == 0, "cf_dcn_v2_f16x3: bad out_stride");
  CF_REQUIRE(a->act == CF_ACT_NONE || a->act == CF_ACT_RELU, "cf_dcn_v2_f16x3: act=%d unsupported", a->act);
  CF_REQUIRE(a->out_scale > 0.0f, "cf_dcn_v2_f16x3: out_scale missing");
  const long M = (long)a->B * a->H * a->W;
  CF_REQUIRE(M > 0 && M * a->C < (1L << 31), "cf_dcn_v2_f16x3: bad geometry / tensor too large");
  DcnF k{};
  k.x = a->x; k.om = a->offmask; k.weight = reinterpret_cast<const unsigned char*>(a->weight);
  k.bias = a->bias; k.out = a->out;
  k.om_stride = a->om_stride; k.H = a->H; k.W = a->W; k.C = a->C;
  k.n_chunks = 9 * a->C / 32;
  k.chunks_per_tap = a->C / 32;
  k.out_stride = a->out_stride; k.act = a->act; k.M = (int)M; k.N = a->N;
  k.n_rt = a->N_pad / 32;
  k.out_scale = a->out_scale;
  k.in_scale = cf_resolve_in_scale(a->in_scale);
  k.mx_scale = cf_resolve_in_scale(a->mx_scale);
  CF_REQUIRE(k.in_scale > 0.0f && k.mx_scale > 0.0f, "cf_dcn_v2_f16x3: in_scale / mx_scale must be 0 (= 16) or a power of two");
  k.out_split = static_cast<unsigned*>(a->out_split_bf16);
  k.split_stride = a->split_stride;
  k.out_mx = static_cast<unsigned char*>(a->out_mx);
  CF_REQUIRE(!a->out_mx || (a->N == 64 && a->N_pad == 64 && (a->N & 3) == 0),
             "cf_dcn_v2_f16x3: the mx output is the 64-channel feature map's (N = N_pad = 64)");
  CF_REQUIRE(!a->out_split_bf16 || (a->split_stride >= a->N && a->split_stride % 8 == 0 && a->N % 4 == 0),
             "cf_dcn_v2_f16x3: split output needs N %% 4 == 0 and a plane stride >= N that is a multiple of 8");
  hipStream_t st = (hipStream_t)stream;
  // K split for small maps, when the caller provides the workspace (decided per image geometry, never
  // by the batch size: it changes the summation order, and a shard has to reproduce the full batch)
  const unsigned ks = a->workspace ? (unsigned)dcn_k_split(a->H, a->W, k.n_chunks, a->N_pad) : 1u;
  CF_REQUIRE(ks == 1 || (!a->out_split_bf16 && !a->out_mx), "cf_dcn_v2_f16x3: the split-bf16 / mx outputs are not available on K-split maps");
  CF_REQUIRE(ks == 1 || a->workspace_bytes >= (size_t)ks * M * a->N_pad * sizeof(float),
             "cf_dcn_v2_f16x3: workspace of %zu bytes is smaller than cf_dcn_v2_workspace_bytes(...)", a->workspace_bytes);
  CF_REQUIRE(ks == 1 || !gs || a->workspace_bytes >= (size_t)n_groups * ks * M * a->N_pad * sizeof(float),
             "cf_dcn_v2_f16x3_grouped: workspace of %zu bytes is smaller than n_groups x cf_dcn_v2_workspace_bytes(...)", a->workspace_bytes);
  k.partial = static_cast<float*>(a->workspace);
  DcnG g{};
  DcnRG rg{};
  const long G = gs ? n_groups : 1;
  g.M_all = (int)(G * M);
  for (int i = 0; gs && i < n_groups; ++i) {
    g.x[i] = gs[i]->x;
    g.weight[i] = reinterpret_cast<const unsigned char*>(gs[i]->weight);
    g.bias[i] = rg.bias[i] = gs[i]->bias;
    g.in_scale[i] = cf_resolve_in_scale(gs[i]->in_scale);
    g.out_scale[i] = rg.out_scale[i] = gs[i]->out_scale;
    CF_REQUIRE(g.in_scale[i] > 0.0f, "cf_dcn_v2_f16x3_grouped: in_scale must be 0 (= 16) or a power of two");
  }
  k.mask_activated = a->mask_activated;
  CF_REQUIRE(!a->out_mx || (a->N & 3) == 0, "cf_dcn_v2_f16x3: the mx output is written by the whole-row epilogue (N %% 4 == 0)");
  const DcnForm f = dcn_pick(M, a->N, a->N_pad, ks, G);
  if (report) {
    const int32_t v[9] = {f.WC, f.WP, f.RT, f.COAL, f.CT, (int32_t)(f.tiles * G), (int32_t)f.grid_y, (int32_t)f.ks, (int32_t)f.tiles};
    for (int i = 0; i < 9; ++i) report[i] = v[i];
    return CF_OK;
  }
  bool launched = false;
#define X(WC, WP, RT, COAL, CT, HAS_GRP) launched = launched || dcn_launch_if<WC, WP, RT, COAL, CT, HAS_GRP>(f, k, gs ? &g : nullptr, n_groups, st);
  CF_DCN_TILES(X)
#undef X
  CF_REQUIRE(launched, "cf_dcn_v2_f16x3: the picked form <%d, %d, %d, %d, %d>%s is not instantiated", f.WC, f.WP, f.RT, f.COAL, f.CT, gs ? " (grouped)" : "");
  if (ks > 1) {
    const int ns4 = k.n_rt * 32 / 4;
    const long MN4 = G * M * ns4;
    const long blocks = (MN4 + 255) / 256;
    const dim3 rgrid((unsigned)(blocks < 65536 ? blocks : 65536));
    if (gs)
      hipLaunchKernelGGL(dcn_reduce_grouped_kernel, rgrid, dim3(256), 0, st, k.partial, (int)ks, MN4, ns4, a->N, (int)M, rg, a->act,
                         a->out, a->out_stride);
    else
      hipLaunchKernelGGL(dcn_reduce_kernel, rgrid, dim3(256), 0, st, k.partial,
                         (int)ks, MN4, ns4, a->N, a->bias, a->out_scale, a->act, a->out, a->out_stride);
  }
  return cf_check_launch(gs ? "cf_dcn_v2_f16x3_grouped" : "cf_dcn_v2_f16x3");
}

extern "C" int cf_dcn_v2_f16x3(const cf_dcn_args* a, void* stream) { return dcn_f16x3_impl(a, nullptr, 1, stream); }

static int dcn_f16x3_grouped_impl(const cf_dcn_args* const* gs, int32_t n_groups, void* stream, int32_t* report) {
  CF_REQUIRE(gs != nullptr && n_groups >= 1 && n_groups <= CF_MAX_GROUPS, "cf_dcn_v2_f16x3_grouped: n_groups=%d outside 1..%d", n_groups, CF_MAX_GROUPS);
  for (int g = 0; g < n_groups; ++g) CF_REQUIRE(gs[g] != nullptr, "cf_dcn_v2_f16x3_grouped: group %d is null", g);
  if (n_groups == 1) return dcn_f16x3_impl(gs[0], nullptr, 1, stream, report);
  const cf_dcn_args* a = gs[0];
  CF_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->om_stride > 0 && a->out_stride > 0 && a->N > 0, "cf_dcn_v2_f16x3_grouped: bad geometry");
  const size_t M = (size_t)a->B * a->H * a->W;
  CF_REQUIRE(M * n_groups < (1UL << 31), "cf_dcn_v2_f16x3_grouped: tensor too large");
  CF_REQUIRE((a->N & 3) == 0, "cf_dcn_v2_f16x3_grouped: N=%d must be a multiple of 4 (whole-row epilogue)", a->N);
  CF_REQUIRE(a->N_pad <= 128, "cf_dcn_v2_f16x3_grouped: N_pad=%d above 128 has no grouped form", a->N_pad);
  for (int g = 0; g < n_groups; ++g) {
    const cf_dcn_args* b = gs[g];
    CF_REQUIRE(!b->out_split_bf16 && !b->out_mx, "cf_dcn_v2_f16x3_grouped: group %d: the split-bf16 / mx outputs are not available with n_groups > 1", g);
    CF_REQUIRE(b->x && b->weight && b->bias && b->offmask && b->out && b->out_scale > 0.0f, "cf_dcn_v2_f16x3_grouped: group %d: null buffer / out_scale missing", g);
    CF_REQUIRE(b->B == a->B && b->H == a->H && b->W == a->W && b->C == a->C && b->N == a->N && b->N_pad == a->N_pad &&
                   b->om_stride == a->om_stride && b->out_stride == a->out_stride && b->act == a->act && b->mask_activated == a->mask_activated,
               "cf_dcn_v2_f16x3_grouped: group %d differs from group 0 in geometry", g);
    CF_REQUIRE(b->offmask == a->offmask + g * M * a->om_stride && b->out == a->out + g * M * a->out_stride,
               "cf_dcn_v2_f16x3_grouped: group %d must use rows [g M, (g + 1) M) of group 0's offmask / out buffers", g);
  }
  return dcn_f16x3_impl(a, gs, n_groups, stream, report);
}

extern "C" int cf_dcn_v2_f16x3_grouped(const cf_dcn_args* const* gs, int32_t n_groups, void* stream) {
  return dcn_f16x3_grouped_impl(gs, n_groups, stream, nullptr);
}

extern "C" int cf_dcn_v2_f16x3_form(const cf_dcn_args* const* gs, int32_t n_groups, int32_t* form) {
  CF_REQUIRE(form != nullptr, "cf_dcn_v2_f16x3_form: null output");
  return dcn_f16x3_grouped_impl(gs, n_groups, nullptr, form);
}

extern "C" size_t cf_dcn_v2_workspace_bytes(int B, int H, int W, int C, int N_pad) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N_pad <= 0) return 0;
  const int ks = dcn_k_split(H, W, 9 * C / 32, N_pad);
  return ks > 1 ? (size_t)ks * B * H * W * N_pad * sizeof(float) : 0;
}
