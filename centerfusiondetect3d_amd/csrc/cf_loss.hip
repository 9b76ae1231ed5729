// The criterion (GenericLoss of the reference's model/genericLoss.py + losses.py, one output layer) on the device:
// forward in two launches, backward in two, no host sync, no float atomics in the forward.  Semantics: include/cf_hip.h.
//
// Reductions have ONE order: per thread over its grid-stride elements, wave shuffles, the waves' sums through LDS added in
// wave order, and (heat map only) the workgroups' partial sums added by the object kernel in the same way - so the loss
// values are bitwise reproducible.  The backward scatters with float atomic adds into zero-filled maps.
#include "cf_common.h"

#define LOSS_DENSE_THREADS 256
#define LOSS_MAX_PARTIALS 1024   // workgroups of the dense forward pass = threads of the object kernel (one partial each)
#define LOSS_OBJ_THREADS 1024
#define LOSS_BWD_THREADS 256

// stats layout: [0] heat normaliser (1 / sum m, or 1), [1] sum m, [2] rows with m != 0; head i at 4 + 4 i:
//   L1 / BCE: [0] 1 / divisor      L1_UNC: [0] 1 / rows averaged over, [1] 1 when that is every row
//   BINROT:   [0] 1 / rows with m != 0, [1] 1 / rows with rotbin[0] != 0, [2] the same for rotbin[1]   (0 = term absent)
#define STAT_HEAD(i) (4 + 4 * (i))

__device__ __forceinline__ float loss_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Sum over the workgroup, the same value in every thread.  lds: NT / 64 floats.
template <int NT>
__device__ __forceinline__ float loss_block_sum(float v, float* lds) {
  v = loss_wave_sum(v);
  __syncthreads();   // the previous sum's readers are done with lds
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) r += lds[i];
  return r;
}

__device__ __forceinline__ float loss_neg_term(float p, float g) {
  const float q = 1.f - g, q2 = q * q;
  return log1pf(-p) * (p * p) * (q2 * q2);
}

// d/dp of the negative term
__device__ __forceinline__ float loss_neg_grad(float p, float g) {
  const float q = 1.f - g, q2 = q * q;
  return (2.f * p * log1pf(-p) - (p * p) / (1.f - p)) * (q2 * q2);
}

__device__ __forceinline__ float loss_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ float loss_lse2(float a, float b) { return fmaxf(a, b) + log1pf(expf(-fabsf(a - b))); }

__device__ __forceinline__ float loss_smooth_l1(float d) {
  const float ad = fabsf(d);
  return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

__device__ __forceinline__ float loss_smooth_l1_grad(float d) { return fabsf(d) < 1.f ? d : loss_sign(d); }

// One object row under the layer mask: image b, pixel (clamped), mask m, class (clamped); -> lm.
struct LossRow {
  int b;
  int pix;
  int cls;
  float m;
  bool lm;
};

__device__ __forceinline__ LossRow loss_row(const cf_loss_args& a, int r) {
  LossRow o;
  o.b = r / a.M;
  o.lm = (a.wh[2 * r] * a.wh[2 * r + 1]) / a.out_area > 0.f;
  o.pix = 0;
  o.cls = 0;
  o.m = 0.f;
  if (o.lm) {
    const long hw = (long)a.h * a.w;
    long p = (long)(int)a.centers[2 * r + 1] * a.w + (long)(int)a.centers[2 * r];
    p = p < 0 ? 0 : (p >= hw ? hw - 1 : p);
    long c = a.cls[r];
    c = c < 0 ? 0 : (c >= a.C ? a.C - 1 : c);
    o.pix = (int)p;
    o.cls = (int)c;
    o.m = a.mask[r];
  }
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward 1: the negative focal term over the whole map, one partial sum per workgroup
__global__ __launch_bounds__(LOSS_DENSE_THREADS) void cf_loss_heat_fwd_kernel(const float* __restrict__ p,
                                                                              const float* __restrict__ gt, long n, long nvec,
                                                                              float* __restrict__ partial) {
  __shared__ float lds[LOSS_DENSE_THREADS / 64];
  const long stride = (long)gridDim.x * LOSS_DENSE_THREADS;
  const long first = (long)blockIdx.x * LOSS_DENSE_THREADS + threadIdx.x;
  float acc = 0.f;
  for (long i = first; i < nvec; i += stride) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 g = reinterpret_cast<const f32x4*>(gt)[i];
    acc += (loss_neg_term(a.x, g.x) + loss_neg_term(a.y, g.y)) + (loss_neg_term(a.z, g.z) + loss_neg_term(a.w, g.w));
  }
  for (long i = nvec * 4 + first; i < n; i += stride) acc += loss_neg_term(p[i], gt[i]);
  const float s = loss_block_sum<LOSS_DENSE_THREADS>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// forward 2: ONE workgroup over the B*M objects; every head's term, every count, the branches, the total
__global__ __launch_bounds__(LOSS_OBJ_THREADS) void cf_loss_obj_fwd_kernel(const cf_loss_args a, int n_partial) {
  __shared__ float lds[LOSS_OBJ_THREADS / 64];
  const int tid = threadIdx.x;
  const int R = a.B * a.M;
  const long hw = (long)a.h * a.w;
  const float* partial = static_cast<const float*>(a.workspace);
  constexpr int NT = LOSS_OBJ_THREADS;

  const float neg = loss_block_sum<NT>(tid < n_partial ? partial[tid] : 0.f, lds);

  float pos = 0.f, sm = 0.f, cnt = 0.f;
  for (int r = tid; r < R; r += NT) {
    const LossRow o = loss_row(a, r);
    if (a.layer_mask) a.layer_mask[r] = o.lm ? 1 : 0;
    const float p = a.heat[((long)o.b * a.C + o.cls) * hw + o.pix];
    const float q = 1.f - p;
    pos += logf(p) * (q * q) * o.m;
    sm += o.m;
    cnt += o.m != 0.f ? 1.f : 0.f;
  }
  pos = loss_block_sum<NT>(pos, lds);
  sm = loss_block_sum<NT>(sm, lds);
  cnt = loss_block_sum<NT>(cnt, lds);
  const float heat_loss = sm == 0.f ? -neg : -(pos + neg) / sm;
  float total = heat_loss * a.heat_weight;
  if (tid == 0) {
    a.losses[0] = heat_loss;
    a.stats[0] = sm == 0.f ? 1.f : 1.f / sm;
    a.stats[1] = sm;
    a.stats[2] = cnt;
    a.stats[3] = 0.f;
  }

  for (int hd = 0; hd < a.n_heads; ++hd) {
    const cf_loss_head& H = a.head[hd];
    const int Ch = H.channels;
    float value = 0.f, to_total = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (H.kind == CF_LOSS_L1) {
      float acc = 0.f;
      for (int r = tid; r < R; r += NT) {
        const LossRow o = loss_row(a, r);
        for (int c = 0; c < Ch; ++c) {
          const float pred = H.map[((long)o.b * Ch + c) * hw + o.pix];
          const float t = o.lm ? H.target[(long)r * Ch + c] : 0.f;
          acc += fabsf(pred * o.m - t * o.m);
        }
      }
      acc = loss_block_sum<NT>(acc, lds);
      const float n = sm == 0.f ? 1e7f : (float)Ch * sm;
      value = to_total = acc / n;
      s0 = 1.f / n;
    } else if (H.kind == CF_LOSS_L1_UNC) {
      float al = 0.f, ae = 0.f, aall = 0.f;
      for (int r = tid; r < R; r += NT) {
        const LossRow o = loss_row(a, r);
        const float pred = H.map[(long)o.b * hw + o.pix];
        const float t = o.lm ? H.target[r] : 0.f;
        const float l = fabsf(pred * o.m - t * o.m);
        const float u = fminf(fmaxf(H.unc[(long)o.b * hw + o.pix], -10.f), 10.f);
        const float e = l * expf(-u) + u;
        aall += e;
        if (o.m != 0.f) {
          al += l;
          ae += e;
        }
      }
      al = loss_block_sum<NT>(al, lds);
      ae = loss_block_sum<NT>(ae, lds);
      aall = loss_block_sum<NT>(aall, lds);
      const bool all = sm == 0.f;   // the reference branches on the sum; with no m != 0 row |d| is 0 everywhere
      const float n = all ? (float)R : cnt;
      value = all ? 0.f : al / n;
      to_total = (all ? aall : ae) / n;
      s0 = 1.f / n;
      s1 = all ? 1.f : 0.f;
    } else if (H.kind == CF_LOSS_BINROT) {
      float ce = 0.f, r0 = 0.f, c0 = 0.f, r1 = 0.f, c1 = 0.f;
      for (int r = tid; r < R; r += NT) {
        const LossRow o = loss_row(a, r);
        float x[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = H.map[((long)o.b * 8 + c) * hw + o.pix];
        const bool b0 = o.lm && H.rotbin[2 * r] != 0, b1 = o.lm && H.rotbin[2 * r + 1] != 0;
        if (o.m != 0.f) ce += (loss_lse2(x[0], x[1]) - (b0 ? x[1] : x[0])) + (loss_lse2(x[4], x[5]) - (b1 ? x[5] : x[4]));
        if (b0) {
          const float t = H.target[2 * r];
          r0 += loss_smooth_l1(x[2] - sinf(t)) + loss_smooth_l1(x[3] - cosf(t));
          c0 += 1.f;
        }
        if (b1) {
          const float t = H.target[2 * r + 1];
          r1 += loss_smooth_l1(x[6] - sinf(t)) + loss_smooth_l1(x[7] - cosf(t));
          c1 += 1.f;
        }
      }
      ce = loss_block_sum<NT>(ce, lds);
      r0 = loss_block_sum<NT>(r0, lds);
      c0 = loss_block_sum<NT>(c0, lds);
      r1 = loss_block_sum<NT>(r1, lds);
      c1 = loss_block_sum<NT>(c1, lds);
      if (sm != 0.f) {
        value = cnt > 0.f ? ce / cnt : 0.f;
        if (c0 > 0.f) value += r0 / c0;
        if (c1 > 0.f) value += r1 / c1;
        s0 = cnt > 0.f ? 1.f / cnt : 0.f;
        s1 = c0 > 0.f ? 1.f / c0 : 0.f;
        s2 = c1 > 0.f ? 1.f / c1 : 0.f;
      }
      to_total = value;
    } else {   // CF_LOSS_BCE
      float acc = 0.f, sam = 0.f;
      for (int r = tid; r < R; r += NT) {
        const LossRow o = loss_row(a, r);
        for (int c = 0; c < Ch; ++c) {
          const float x = H.map[((long)o.b * Ch + c) * hw + o.pix];
          const float t = o.lm ? H.target[(long)r * Ch + c] : 0.f;
          const float am = o.lm ? H.mask[(long)r * Ch + c] : 0.f;
          acc += am * (fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))));
          sam += am;
        }
      }
      acc = loss_block_sum<NT>(acc, lds);
      sam = loss_block_sum<NT>(sam, lds);
      const float n = sam == 0.f ? 1e7f : sam;
      value = to_total = acc / n;
      s0 = 1.f / n;
    }
    total += to_total * H.weight;
    if (tid == 0) {
      a.losses[1 + hd] = value;
      float* st = a.stats + STAT_HEAD(hd);
      st[0] = s0;
      st[1] = s1;
      st[2] = s2;
      st[3] = s3;
    }
  }
  if (tid == 0) {
    a.losses[1 + a.n_heads] = total;
    a.losses[2 + a.n_heads] = 0.f;
    if (a.total) *a.total = total;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward 1: the heat map's gradient from the negative term, every element written
__global__ __launch_bounds__(LOSS_DENSE_THREADS) void cf_loss_heat_bwd_kernel(const float* __restrict__ p,
                                                                              const float* __restrict__ gt, long n, long nvec,
                                                                              const float* __restrict__ stats,
                                                                              const float* __restrict__ grad_out,
                                                                              float heat_weight, float* __restrict__ g) {
  const float k = -(*grad_out) * heat_weight * stats[0];
  const long stride = (long)gridDim.x * LOSS_DENSE_THREADS;
  const long first = (long)blockIdx.x * LOSS_DENSE_THREADS + threadIdx.x;
  for (long i = first; i < nvec; i += stride) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 t = reinterpret_cast<const f32x4*>(gt)[i];
    f32x4 o;
    o.x = k * loss_neg_grad(a.x, t.x);
    o.y = k * loss_neg_grad(a.y, t.y);
    o.z = k * loss_neg_grad(a.z, t.z);
    o.w = k * loss_neg_grad(a.w, t.w);
    reinterpret_cast<f32x4*>(g)[i] = o;
  }
  for (long i = nvec * 4 + first; i < n; i += stride) g[i] = k * loss_neg_grad(p[i], gt[i]);
}

__device__ __forceinline__ void loss_add(float* p, float v) {
  if (v != 0.f) atomicAdd(p, v);   // a row that contributes nothing leaves its pixel untouched
}

// backward 2: grid (rows / 256, n_heads + 1); blockIdx.y = head, the last one = the positive focal terms
__global__ __launch_bounds__(LOSS_BWD_THREADS) void cf_loss_obj_bwd_kernel(const cf_loss_args a) {
  const int r = blockIdx.x * LOSS_BWD_THREADS + threadIdx.x;
  if (r >= a.B * a.M) return;
  const int hd = blockIdx.y;
  const long hw = (long)a.h * a.w;
  const float go = *a.grad_out;
  const LossRow o = loss_row(a, r);
  if (hd == a.n_heads) {
    if (!a.gheat) return;
    const long at = ((long)o.b * a.C + o.cls) * hw + o.pix;
    const float p = a.heat[at], q = 1.f - p;
    loss_add(a.gheat + at, -go * a.heat_weight * a.stats[0] * o.m * ((q * q) / p - 2.f * q * logf(p)));
    return;
  }
  const cf_loss_head& H = a.head[hd];
  const float* st = a.stats + STAT_HEAD(hd);
  const float k = go * H.weight;
  const int Ch = H.channels;
  if (H.kind == CF_LOSS_L1) {
    if (!H.gmap || o.m == 0.f) return;
    for (int c = 0; c < Ch; ++c) {
      const long at = ((long)o.b * Ch + c) * hw + o.pix;
      const float d = H.map[at] * o.m - H.target[(long)r * Ch + c] * o.m;   // m != 0 implies lm
      loss_add(H.gmap + at, k * st[0] * o.m * loss_sign(d));
    }
  } else if (H.kind == CF_LOSS_L1_UNC) {
    if (st[1] == 0.f && o.m == 0.f) return;   // averaged over the rows with m != 0 only
    const long at = (long)o.b * hw + o.pix;
    const float t = o.lm ? H.target[r] : 0.f;
    const float d = H.map[at] * o.m - t * o.m;
    const float uraw = H.unc[at];
    const float u = fminf(fmaxf(uraw, -10.f), 10.f);
    const float sg = expf(-u);
    if (H.gmap) loss_add(H.gmap + at, k * st[0] * o.m * loss_sign(d) * sg);
    if (H.gunc && uraw >= -10.f && uraw <= 10.f) loss_add(H.gunc + at, k * st[0] * (1.f - fabsf(d) * sg));
  } else if (H.kind == CF_LOSS_BINROT) {
    if (!H.gmap || !o.lm) return;   // without lm: m = 0 and rotbin = 0, the row is in no term
    float x[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = H.map[((long)o.b * 8 + c) * hw + o.pix];
    const bool b0 = H.rotbin[2 * r] != 0, b1 = H.rotbin[2 * r + 1] != 0;
    float* g = H.gmap + (long)o.b * 8 * hw + o.pix;
    if (o.m != 0.f && st[0] != 0.f) {
      const float p1 = 1.f / (1.f + expf(x[0] - x[1])), p5 = 1.f / (1.f + expf(x[4] - x[5]));
      const float kb = k * st[0];
      loss_add(g + 0 * hw, kb * (b0 ? 1.f - p1 : -p1));   // softmax - one-hot; p1 / p5: the probability of class 1
      loss_add(g + 1 * hw, kb * (b0 ? p1 - 1.f : p1));
      loss_add(g + 4 * hw, kb * (b1 ? 1.f - p5 : -p5));
      loss_add(g + 5 * hw, kb * (b1 ? p5 - 1.f : p5));
    }
    if (b0 && st[1] != 0.f) {
      const float t = H.target[2 * r];
      loss_add(g + 2 * hw, k * st[1] * loss_smooth_l1_grad(x[2] - sinf(t)));
      loss_add(g + 3 * hw, k * st[1] * loss_smooth_l1_grad(x[3] - cosf(t)));
    }
    if (b1 && st[2] != 0.f) {
      const float t = H.target[2 * r + 1];
      loss_add(g + 6 * hw, k * st[2] * loss_smooth_l1_grad(x[6] - sinf(t)));
      loss_add(g + 7 * hw, k * st[2] * loss_smooth_l1_grad(x[7] - cosf(t)));
    }
  } else {   // CF_LOSS_BCE
    if (!H.gmap || !o.lm) return;
    for (int c = 0; c < Ch; ++c) {
      const float am = H.mask[(long)r * Ch + c];
      if (am == 0.f) continue;
      const long at = ((long)o.b * Ch + c) * hw + o.pix;
      loss_add(H.gmap + at, k * st[0] * am * (cf_sigmoid(H.map[at]) - H.target[(long)r * Ch + c]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static int loss_dense_blocks(long n) {
  long b = (n / 4 + LOSS_DENSE_THREADS - 1) / LOSS_DENSE_THREADS;
  return (int)(b < 1 ? 1 : (b > LOSS_MAX_PARTIALS ? LOSS_MAX_PARTIALS : b));
}

static int loss_check(const cf_loss_args* a, const char* what) {
  CF_REQUIRE(a, "%s: args is NULL", what);
  CF_REQUIRE(a->B > 0 && a->C > 0 && a->h > 0 && a->w > 0 && a->M > 0, "%s: B, C, h, w, M must be positive", what);
  CF_REQUIRE((long)a->B * a->C * a->h * a->w < (1L << 40) && (long)a->h * a->w < (1L << 31) && (long)a->B * a->M < (1L << 24),
             "%s: shape out of range", what);
  CF_REQUIRE(a->n_heads >= 0 && a->n_heads <= CF_LOSS_MAX_HEADS, "%s: n_heads must be 0..%d", what, CF_LOSS_MAX_HEADS);
  CF_REQUIRE(a->out_area > 0.f, "%s: out_area must be positive", what);
  CF_REQUIRE(a->heat && a->heat_gt && a->centers && a->wh && a->mask && a->cls && a->stats,
             "%s: heat, heat_gt, centers, wh, mask, cls and stats are required", what);
  for (int i = 0; i < a->n_heads; ++i) {
    const cf_loss_head& H = a->head[i];
    CF_REQUIRE(H.kind >= CF_LOSS_L1 && H.kind <= CF_LOSS_BCE, "%s: head %d: unknown kind %d", what, i, H.kind);
    CF_REQUIRE(H.map && H.target, "%s: head %d: map and target are required", what, i);
    CF_REQUIRE(H.channels > 0 && H.channels <= 1024, "%s: head %d: channels out of range", what, i);
    CF_REQUIRE(H.kind != CF_LOSS_L1_UNC || (H.channels == 1 && H.unc), "%s: head %d: L1_UNC needs one channel and unc", what, i);
    CF_REQUIRE(H.kind != CF_LOSS_BINROT || (H.channels == 8 && H.rotbin), "%s: head %d: BINROT needs eight channels and rotbin", what, i);
    CF_REQUIRE(H.kind != CF_LOSS_BCE || H.mask, "%s: head %d: BCE needs mask", what, i);
  }
  return CF_OK;
}

static bool loss_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" size_t cf_loss_workspace_bytes(int B, int C, int h, int w) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)loss_dense_blocks((long)B * C * h * w) * sizeof(float);
}

extern "C" int cf_loss_forward(const cf_loss_args* a, void* stream) {
  if (int e = loss_check(a, "cf_loss_forward")) return e;
  CF_REQUIRE(a->losses, "cf_loss_forward: losses is required");
  const long n = (long)a->B * a->C * a->h * a->w;
  const int nblk = loss_dense_blocks(n);
  CF_REQUIRE(a->workspace && a->workspace_bytes >= (size_t)nblk * sizeof(float),
             "cf_loss_forward: workspace must hold cf_loss_workspace_bytes() = %zu bytes", (size_t)nblk * sizeof(float));
  const long nvec = loss_aligned16(a->heat) && loss_aligned16(a->heat_gt) ? n / 4 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cf_loss_heat_fwd_kernel, dim3(nblk), dim3(LOSS_DENSE_THREADS), 0, s, a->heat, a->heat_gt, n, nvec,
                     static_cast<float*>(a->workspace));
  if (int e = cf_check_launch("cf_loss_forward (heat map)")) return e;
  hipLaunchKernelGGL(cf_loss_obj_fwd_kernel, dim3(1), dim3(LOSS_OBJ_THREADS), 0, s, *a, nblk);
  return cf_check_launch("cf_loss_forward (objects)");
}

extern "C" int cf_loss_backward(const cf_loss_args* a, void* stream) {
  if (int e = loss_check(a, "cf_loss_backward")) return e;
  CF_REQUIRE(a->grad_out, "cf_loss_backward: grad_out is required");
  bool any = a->gheat != nullptr;
  for (int i = 0; i < a->n_heads; ++i) any = any || a->head[i].gmap || a->head[i].gunc;
  if (!any) return CF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->gheat) {
    const long n = (long)a->B * a->C * a->h * a->w;
    const long nvec = loss_aligned16(a->heat) && loss_aligned16(a->heat_gt) && loss_aligned16(a->gheat) ? n / 4 : 0;
    hipLaunchKernelGGL(cf_loss_heat_bwd_kernel, dim3(loss_dense_blocks(n)), dim3(LOSS_DENSE_THREADS), 0, s, a->heat,
                       a->heat_gt, n, nvec, a->stats, a->grad_out, a->heat_weight, a->gheat);
    if (int e = cf_check_launch("cf_loss_backward (heat map)")) return e;
  }
  const int R = a->B * a->M;
  hipLaunchKernelGGL(cf_loss_obj_bwd_kernel, dim3((R + LOSS_BWD_THREADS - 1) / LOSS_BWD_THREADS, a->n_heads + 1),
                     dim3(LOSS_BWD_THREADS), 0, s, *a);
  return cf_check_launch("cf_loss_backward (objects)");
}
