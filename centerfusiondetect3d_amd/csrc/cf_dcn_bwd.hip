// Backward of the modulated deformable 3x3 convolution (stride 1, pad 1, dil 1, one group, one offset group) on fp32
// NHWC tensors - what autograd needs behind ops.deform_conv2d.  The sampling rule is the forward's (oracle/dcn_ref.py):
// the open interval (-1, H) x (-1, W), per-corner validity, floor held constant (so the offset gradient at an integer
// position is the right-hand derivative).  Products run on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32): there is
// no activation range to guard and nothing is clamped.
//
//   cf_dcn_v2_bwd_data    gx (float atomics into the <= 4 valid corners, 128-byte rows) and gom (plain stores)
//   cf_dcn_v2_bwd_weight  gw / gbias: K = B*H*W split into slabs, reduced in slab order by a second kernel (bitwise reproducible)
#include "cf_common.h"

namespace {

// one bilinear sample: where its four corners are and what they weigh
struct Sample {
  int base;      // element offset of the (clamped) top-left corner's channel 0 in x
  int dxo, dyo;  // element offsets to the right / lower corner (0 where that corner is clamped onto this one)
  int ok;        // bit 0..3: corner (t,l) (t,r) (b,l) (b,r) lies inside the image (0 for a sample outside the open interval)
  float lh, lw;  // fractional parts
};

__device__ __forceinline__ Sample dcn_sample(int H, int W, int C, int b, int ho, int wo, int tap, float dy, float dx) {
  const int ti = tap / 3, tj = tap - ti * 3;
  const float hf = (float)(ho - 1 + ti) + dy;
  const float wf = (float)(wo - 1 + tj) + dx;
  const bool inside = hf > -1.0f && hf < (float)H && wf > -1.0f && wf < (float)W;
  const float hfl = floorf(hf), wfl = floorf(wf);
  const int hl = inside ? (int)hfl : 0, wl = inside ? (int)wfl : 0;
  const bool t_ok = inside && hl >= 0, b_ok = inside && hl + 1 <= H - 1;
  const bool l_ok = wl >= 0, r_ok = wl + 1 <= W - 1;
  const int y0 = max(hl, 0), x0 = max(wl, 0);
  const int y1 = min(hl + 1, H - 1), x1 = min(wl + 1, W - 1);
  Sample s;
  s.base = ((b * H + y0) * W + x0) * C;
  s.dxo = (max(x1, x0) - x0) * C;
  s.dyo = (max(y1, y0) - y0) * W * C;
  s.ok = (t_ok && l_ok ? 1 : 0) | (t_ok && r_ok ? 2 : 0) | (b_ok && l_ok ? 4 : 0) | (b_ok && r_ok ? 8 : 0);
  s.lh = hf - hfl;
  s.lw = wf - wfl;
  return s;
}

struct BwdData {
  const float* gout;
  const float* weight;
  const float* x;
  const float* om;
  float* gx;
  float* gom;
  int H, W, C, N, M;
};

constexpr int DPX = 32;   // pixels per workgroup of the data kernel (one 32x32 MFMA tile; its waves share them)

// G[pix, c] = sum_o gout[pix, o] W[o, c, tap] per (tap, 32-channel chunk) in the accumulators: the lane holds channel
// c0 + (lane & 31) of 16 pixels, so a half wave reads / adds one 128-byte row of x / gx per corner.  The workgroup has
// min(C / 32, 4) waves, which take the chunks round robin; their gom parts meet in LDS and are added in wave order.
__global__ __launch_bounds__(256) void dcn_bwd_data_kernel(const BwdData p) {
  extern __shared__ float afrag[];                 // [ceil(N / 2)][64]: gout in A-operand order (lane: pixel l & 31, output 2 s + (l >> 5))
  __shared__ f32x4 desc[9 * DPX * 2];              // per (tap, pixel): {base, dxo, dyo, ok} {lh, lw, mask, -}
  __shared__ float gomt[4][DPX * 32];              // per wave: the tile's gom rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;         // min(C / 32, 4) waves: one per chunk, none without work
  const int m0 = blockIdx.x * DPX;
  const int HW = p.H * p.W;
  const int nsteps = (p.N + 1) >> 1;

  for (int i = tid; i < nsteps * 64; i += nt) {
    const int s = i >> 6, l = i & 63;
    const int o = 2 * s + (l >> 5), m = m0 + (l & 31);
    afrag[i] = (o < p.N && m < p.M) ? p.gout[(size_t)m * p.N + o] : 0.0f;
  }
  for (int i = tid; i < 9 * DPX; i += nt) {
    const int tap = i / DPX, r = i - tap * DPX;
    const int m = m0 + r;
    f32x4 dA = {__int_as_float(0), __int_as_float(0), __int_as_float(0), __int_as_float(0)};
    f32x4 dB = {0.0f, 0.0f, 0.0f, 0.0f};
    if (m < p.M) {
      const int b = m / HW, rem = m - b * HW;
      const int ho = rem / p.W, wo = rem - ho * p.W;
      const float* om = p.om + (size_t)m * 32;
      const Sample s = dcn_sample(p.H, p.W, p.C, b, ho, wo, tap, om[2 * tap], om[2 * tap + 1]);
      dA = f32x4{__int_as_float(s.base), __int_as_float(s.dxo), __int_as_float(s.dyo), __int_as_float(s.ok)};
      dB = f32x4{s.lh, s.lw, om[18 + tap], 0.0f};
    }
    desc[2 * i] = dA;
    desc[2 * i + 1] = dB;
  }
  for (int i = tid; i < 4 * DPX * 32; i += nt) (&gomt[0][0])[i] = 0.0f;
  __syncthreads();

  const int half = lane >> 5, cl = lane & 31;
  const int nch = p.C >> 5;
  for (int tap = 0; tap < 9; ++tap) {
    // a tap none of the tile's samples reaches contributes nothing
    const int ok_l = __float_as_int(desc[2 * (tap * DPX + cl)][3]);
    if (__ballot(ok_l != 0) == 0) continue;
    float pm[16], pdy[16], pdx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) pm[r] = pdy[r] = pdx[r] = 0.0f;
    for (int ch = wave; ch < nch; ch += nw) {
      const int c = ch * 32 + cl;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      const float* wp = p.weight + (size_t)c * 9 + tap;
      // eight steps' weights are loaded before their MFMAs (a load per MFMA would wait out its whole latency every step);
      // the steps past the last one read clamped addresses and multiply zeros
      for (int s0 = 0; s0 < nsteps; s0 += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int s = s0 + u, o = 2 * s + half;
          const float wv = wp[(size_t)min(o, p.N - 1) * p.C * 9];
          const float gv = afrag[min(s, nsteps - 1) * 64 + lane];
          bv[u] = o < p.N ? wv : 0.0f;
          av[u] = s < nsteps ? gv : 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);         // (the scheduler would pair each load with its MFMA again)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      }
      // all 64 corner values are loaded before any is used (a pixel at a time would wait out the load latency 16 times): the
      // addresses are clamped into x even where the corner is not valid, so the loads are unconditional
      float xv[16][4];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int px = (r & 3) + 8 * (r >> 2) + 4 * half;
        const f32x4 dA = desc[2 * (tap * DPX + px)];
        const int a0 = __float_as_int(dA[0]) + c, dxo = __float_as_int(dA[1]), dyo = __float_as_int(dA[2]);
        xv[r][0] = p.x[a0];
        xv[r][1] = p.x[a0 + dxo];
        xv[r][2] = p.x[a0 + dyo];
        xv[r][3] = p.x[a0 + dyo + dxo];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int px = (r & 3) + 8 * (r >> 2) + 4 * half;
        const f32x4 dA = desc[2 * (tap * DPX + px)], dB = desc[2 * (tap * DPX + px) + 1];
        const int ok = __float_as_int(dA[3]);
        const float lh = dB[0], lw = dB[1], hh = 1.0f - lh, hw = 1.0f - lw;
        const float v1 = (ok & 1) ? xv[r][0] : 0.0f;
        const float v2 = (ok & 2) ? xv[r][1] : 0.0f;
        const float v3 = (ok & 4) ? xv[r][2] : 0.0f;
        const float v4 = (ok & 8) ? xv[r][3] : 0.0f;
        const float g = acc[r];
        pm[r] += g * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4);
        pdy[r] += g * (hw * (v3 - v1) + lw * (v4 - v2));
        pdx[r] += g * (hh * (v2 - v1) + lh * (v4 - v3));
      }
      // the adds need no loaded value: issued behind ALL the tile's corner loads, which would otherwise each wait (one in-order
      // counter) for the atomics of the pixel before them
      if (p.gx) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int px = (r & 3) + 8 * (r >> 2) + 4 * half;
          const f32x4 dA = desc[2 * (tap * DPX + px)], dB = desc[2 * (tap * DPX + px) + 1];
          const int ok = __float_as_int(dA[3]);
          if (ok == 0) continue;
          const int a0 = __float_as_int(dA[0]) + c, dxo = __float_as_int(dA[1]), dyo = __float_as_int(dA[2]);
          const float lh = dB[0], lw = dB[1], hh = 1.0f - lh, hw = 1.0f - lw;
          const float gm = acc[r] * dB[2];
          if (ok & 1) atomicAdd(p.gx + a0, gm * (hh * hw));
          if (ok & 2) atomicAdd(p.gx + a0 + dxo, gm * (hh * lw));
          if (ok & 4) atomicAdd(p.gx + a0 + dyo, gm * (lh * hw));
          if (ok & 8) atomicAdd(p.gx + a0 + dyo + dxo, gm * (lh * lw));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float a = pm[r], b = pdy[r], d = pdx[r];
#pragma unroll
      for (int sft = 16; sft >= 1; sft >>= 1) {
        a += __shfl_xor(a, sft, 64);
        b += __shfl_xor(b, sft, 64);
        d += __shfl_xor(d, sft, 64);
      }
      if (cl == 0) {
        const int px = (r & 3) + 8 * (r >> 2) + 4 * half;
        const float mk = desc[2 * (tap * DPX + px) + 1][2];
        gomt[wave][px * 32 + 2 * tap] = mk * b;
        gomt[wave][px * 32 + 2 * tap + 1] = mk * d;
        gomt[wave][px * 32 + 18 + tap] = a;
      }
    }
  }
  __syncthreads();
  if (p.gom) {
    for (int i = tid; i < DPX * 32; i += nt) {
      const int m = m0 + (i >> 5);
      if (m >= p.M) break;
      float v = gomt[0][i];
      for (int w = 1; w < nw; ++w) v += gomt[w][i];
      p.gom[(size_t)m0 * 32 + i] = v;
    }
  }
}

struct BwdWeight {
  const float* gout;
  const float* x;
  const float* om;
  float* ws;        // [slabs][9][N][C] partial gw, then [slabs][N] partial gbias
  int H, W, C, N, M;
  int slab_px;      // pixels per slab
  int want_gw;
};

// One wave = one (pixel slab, tap, 32-channel chunk, group of NT 32-output tiles): D[o, c] += gout[pix, o] col[pix, c], two pixels
// per MFMA.  The lane recomputes the column value col[pix, c0 + (lane & 31)] (mask times bilinear sample) from x: nothing is stored.
// The waves of tap 0, chunk 0 also add up their gout operands: the slab's part of gbias.
constexpr int WPAIRS = 4;  // pixel pairs (MFMAs per output tile) per trip of the weight kernel's loop

template <int NT>
__global__ __launch_bounds__(64) void dcn_bwd_weight_kernel(const BwdWeight p) {
  const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
  const int slab = blockIdx.x;
  const int nch = p.C >> 5;
  const int tap = blockIdx.y / nch, ch = blockIdx.y - tap * nch;
  const int o0 = blockIdx.z * NT * 32;
  const int HW = p.H * p.W;
  const int mb = slab * p.slab_px, me = min(mb + p.slab_px, p.M);
  const int c = ch * 32 + cl;
  f32x16 acc[NT];
  float bsum[NT];
  int oc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    bsum[t] = 0.0f;
    oc[t] = min(o0 + t * 32 + cl, p.N - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
  }
  // four pixel pairs per trip, all their loads ahead of their MFMAs (one wave per workgroup: nothing else hides the latency);
  // every address is clamped into the tensors, so the loads are unconditional and what is not wanted is selected away
  for (int m2 = mb; m2 < me; m2 += 2 * WPAIRS) {
    float a[WPAIRS][NT], col[WPAIRS];
    int mc[WPAIRS];
    bool live[WPAIRS];
#pragma unroll
    for (int u = 0; u < WPAIRS; ++u) {
      const int m = m2 + 2 * u + half;
      live[u] = m < me;
      mc[u] = live[u] ? m : me - 1;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float v = p.gout[(size_t)mc[u] * p.N + oc[t]];
        a[u][t] = (live[u] && o0 + t * 32 + cl < p.N) ? v : 0.0f;
      }
      col[u] = 0.0f;
    }
#pragma unroll
    for (int u = 0; u < WPAIRS; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) bsum[t] += a[u][t];
    if (!p.want_gw) continue;
#pragma unroll
    for (int u = 0; u < WPAIRS; ++u) {
      const int b = mc[u] / HW, rem = mc[u] - b * HW;
      const int ho = rem / p.W, wo = rem - ho * p.W;
      const float* om = p.om + (size_t)mc[u] * 32;
      const Sample s = dcn_sample(p.H, p.W, p.C, b, ho, wo, tap, om[2 * tap], om[2 * tap + 1]);
      const float mk = om[18 + tap];
      const int ok = live[u] ? s.ok : 0;
      const int a0 = s.base + c;
      const float hh = 1.0f - s.lh, hw = 1.0f - s.lw;
      const float r1 = p.x[a0], r2 = p.x[a0 + s.dxo], r3 = p.x[a0 + s.dyo], r4 = p.x[a0 + s.dyo + s.dxo];
      const float v1 = (ok & 1) ? r1 : 0.0f;
      const float v2 = (ok & 2) ? r2 : 0.0f;
      const float v3 = (ok & 4) ? r3 : 0.0f;
      const float v4 = (ok & 8) ? r4 : 0.0f;
      col[u] = ok ? mk * (hh * hw * v1 + hh * s.lw * v2 + s.lh * hw * v3 + s.lh * s.lw * v4) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < WPAIRS; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], col[u], acc[t], 0, 0, 0);
  }
  if (p.want_gw) {
    float* wsp = p.ws + ((size_t)slab * 9 + tap) * p.N * p.C;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (o < p.N) wsp[(size_t)o * p.C + c] = acc[t][r];
      }
  }
  if (blockIdx.y == 0) {
    float* wsb = p.ws + (size_t)gridDim.x * 9 * p.N * p.C + (size_t)slab * p.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);     // (even pixels) + (odd pixels): one fixed order
      const int o = o0 + t * 32 + cl;
      if (half == 0 && o < p.N) wsb[o] = v;
    }
  }
}

// gw[o][c][k] = sum over the slabs, in slab order, of ws[slab][k][o][c]; gbias[o] likewise
__global__ __launch_bounds__(256) void dcn_bwd_reduce_kernel(const float* __restrict__ ws, int slabs, int N, int C,
                                                             float* __restrict__ gw, float* __restrict__ gbias) {
  const long per = (long)9 * N * C;
  const long total = (gw ? per : 0) + (gbias ? N : 0);
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total; j += (long)gridDim.x * 256) {
    if (gw && j < per) {
      float v = ws[j];
      for (int z = 1; z < slabs; ++z) v += ws[(size_t)z * per + j];
      const int k = (int)(j / ((long)N * C));
      const long oc = j - (long)k * N * C;
      gw[oc * 9 + k] = v;
    } else {
      const long o = j - (gw ? per : 0);
      const float* wb = ws + (size_t)slabs * per;
      float v = wb[o];
      for (int z = 1; z < slabs; ++z) v += wb[(size_t)z * N + o];
      gbias[o] = v;
    }
  }
}

int bwd_tiles_per_wave(int N) { return N <= 32 ? 1 : N <= 64 ? 2 : 4; }

// pixel slabs of the weight gradient: a function of the geometry alone, so the summation order is too.  At least 256 pixels per
// slab, and no more slabs than give about 2048 waves.
int bwd_slabs(long M, int C, int N) {
  const int nt = bwd_tiles_per_wave(N);
  const long per_slab = 9L * (C / 32) * ((N + 32 * nt - 1) / (32 * nt));
  long s = (M + 255) / 256;
  const long cap = 2048 / per_slab > 1 ? 2048 / per_slab : 1;
  if (s > cap) s = cap;
  return (int)(s < 1 ? 1 : s);
}

int bwd_check(const cf_dcn_bwd_args* a, const char* who) {
  CF_REQUIRE(a != nullptr, "%s: null args", who);
  CF_REQUIRE(a->C > 0 && a->C % 32 == 0, "%s: C=%d not a multiple of 32", who, a->C);
  CF_REQUIRE(a->N > 0 && a->N <= 1024, "%s: N=%d outside 1..1024", who, a->N);
  CF_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "%s: bad geometry", who);
  const long M = (long)a->B * a->H * a->W;
  CF_REQUIRE(M * a->C < (1L << 31) && M * a->N < (1L << 31) && M * 32 < (1L << 31), "%s: tensor too large", who);
  return CF_OK;
}

}  // namespace

extern "C" int cf_dcn_v2_bwd_data(const cf_dcn_bwd_args* a, void* stream) {
  if (int e = bwd_check(a, "cf_dcn_v2_bwd_data")) return e;
  if (!a->gx && !a->gom) return CF_OK;
  CF_REQUIRE(a->gout && a->weight && a->x && a->offmask, "cf_dcn_v2_bwd_data: null buffer");
  BwdData k{};
  k.gout = a->gout; k.weight = a->weight; k.x = a->x; k.om = a->offmask; k.gx = a->gx; k.gom = a->gom;
  k.H = a->H; k.W = a->W; k.C = a->C; k.N = a->N; k.M = a->B * a->H * a->W;
  const size_t dyn = (size_t)((a->N + 1) / 2) * 64 * sizeof(float);
  static CfLdsLimit lds_limit;
  lds_limit.ensure(dcn_bwd_data_kernel, dyn, 32768);
  const unsigned waves = (unsigned)(a->C / 32 < 4 ? a->C / 32 : 4);
  hipLaunchKernelGGL(dcn_bwd_data_kernel, dim3((unsigned)((k.M + DPX - 1) / DPX)), dim3(64 * waves), dyn, (hipStream_t)stream, k);
  return cf_check_launch("cf_dcn_v2_bwd_data");
}

extern "C" size_t cf_dcn_v2_bwd_workspace_bytes(int B, int H, int W, int C, int N) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return 0;
  const int slabs = bwd_slabs((long)B * H * W, C, N);
  return (size_t)slabs * ((size_t)9 * N * C + N) * sizeof(float);
}

extern "C" int cf_dcn_v2_bwd_weight(const cf_dcn_bwd_args* a, void* stream) {
  if (int e = bwd_check(a, "cf_dcn_v2_bwd_weight")) return e;
  if (!a->gw && !a->gbias) return CF_OK;
  CF_REQUIRE(a->gout && (!a->gw || (a->x && a->offmask)), "cf_dcn_v2_bwd_weight: null buffer");
  CF_REQUIRE(a->workspace && a->workspace_bytes >= cf_dcn_v2_bwd_workspace_bytes(a->B, a->H, a->W, a->C, a->N),
             "cf_dcn_v2_bwd_weight: workspace of %zu bytes is smaller than cf_dcn_v2_bwd_workspace_bytes(...)", a->workspace_bytes);
  const long M = (long)a->B * a->H * a->W;
  const int slabs = bwd_slabs(M, a->C, a->N);
  BwdWeight k{};
  k.gout = a->gout; k.x = a->x; k.om = a->offmask; k.ws = static_cast<float*>(a->workspace);
  k.H = a->H; k.W = a->W; k.C = a->C; k.N = a->N; k.M = (int)M;
  k.slab_px = (int)((M + slabs - 1) / slabs);
  k.slab_px += k.slab_px & 1;                       // (two pixels per MFMA: slabs start on an even pixel)
  k.want_gw = a->gw != nullptr;
  const int nt = bwd_tiles_per_wave(a->N);
  const dim3 grid((unsigned)slabs, k.want_gw ? (unsigned)(9 * (a->C / 32)) : 1u, (unsigned)((a->N + 32 * nt - 1) / (32 * nt)));
  hipStream_t st = (hipStream_t)stream;
  if (nt == 1) hipLaunchKernelGGL(dcn_bwd_weight_kernel<1>, grid, dim3(64), 0, st, k);
  else if (nt == 2) hipLaunchKernelGGL(dcn_bwd_weight_kernel<2>, grid, dim3(64), 0, st, k);
  else hipLaunchKernelGGL(dcn_bwd_weight_kernel<4>, grid, dim3(64), 0, st, k);
  const long total = (a->gw ? 9L * a->N * a->C : 0) + (a->gbias ? a->N : 0);
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(dcn_bwd_reduce_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, k.ws, slabs,
                     a->N, a->C, a->gw, a->gbias);
  return cf_check_launch("cf_dcn_v2_bwd_weight");
}
