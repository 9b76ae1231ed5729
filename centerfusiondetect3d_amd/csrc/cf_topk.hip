// Peak top-K of the CenterFusion forward (optionally behind the 3x3 equality NMS) and the 64-bit checksum that guards peaks
// computed beside the forward.
//
// Integer / compare kernels bounded by HBM and LDS, not by the MFMA pipe.  TOPK_SLICES slice workgroups per image + a merge:
// the per-image working set (10x112x200 scores = 896 KB) is L2-resident after the first pass, and the top-K order is
// resolved inside LDS.  Built with -ffp-contract=off like the rest of the index path.
#include "cf_topk.h"

namespace {
// score of flat element i = (c, y, x) of one image; with NMS: heat * (maxpool3x3(heat) == heat)
template <bool NMS>
__device__ __forceinline__ float peak_value(const float* __restrict__ img, int i, int H, int W) {
  const float v = img[i];
  if (!NMS) return v;
  const int HW = H * W;
  const int c = i / HW, pix = i - c * HW;
  const int y = pix / W, x = pix - y * W;
  const float* pl = img + (size_t)c * HW;
  float m = v;
  const int y0 = y > 0 ? y - 1 : y, y1 = y < H - 1 ? y + 1 : y;
  const int x0 = x > 0 ? x - 1 : x, x1 = x < W - 1 ? x + 1 : x;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) m = fmaxf(m, pl[yy * W + xx]);
  return (m == v) ? v : v * 0.0f;
}

// heat * (maxpool3x3(heat) == heat) as its own fully parallel pass (cf_topk_peaks, nms == 2): one
// thread per element, rows of the 3x3 window served by L1/L2.
__global__ __launch_bounds__(256) void nms_kernel(const float* __restrict__ heat, float* __restrict__ out, int H,
                                                  int W, long total) {
  const long N = (long)H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long plane = i / N;
    out[i] = peak_value<true>(heat + plane * N, (int)(i - plane * N), H, W);
  }
}

// Pass 1: top-K of one SLICE of one image (TOPK_SLICES workgroups per image), as sorted 64-bit keys (cf_topk.h).  Every
// element of the image's top-K is in its slice's top-K, so pass 2 only has to merge TOPK_SLICES * K keys.
//  A. every thread takes the max of its strided share -> the K-th largest of the 256 local maxima
//     is a lower bound L of the slice's K-th largest element (at least K elements are >= L);
//  B. elements > L are collected into LDS; if fewer than K, the missing ones are the elements == L
//     with the smallest indices, taken by an index-ordered block scan (the common case on real heat
//     maps: the clamp plateau at 1e-4 ties everywhere);
//  C. the candidates are ordered: up to 1024 of them by RANK COUNTING (every key counts the keys above it - the keys
//     are unique - and the ones ranked below K are written straight to their place: one pass over LDS, one barrier,
//     against the ~45 barrier-separated passes of a bitonic sort), more than that (adversarial inputs) by the sort.
// If more than 4096 elements exceed L (adversarial input), the exact K-th value is found by a
// 4 x 8-bit radix select and step B is repeated with it.
// (a device function of a TOPK_THREADS workgroup: slice `slice` of image `img_i` -> out_keys + (img_i * TOPK_SLICES + slice) * K;
//  the kernel below runs one slice per workgroup, topk_fallback_kernel all slices of an image one after the other)
template <bool NMS>
__device__ __forceinline__ void topk_slice_body(const float* __restrict__ heat, int C, int H, int W, int K,
                                                uint64_t* __restrict__ out_keys, int img_i, int slice) {
  __shared__ __attribute__((aligned(16))) uint64_t keys[TOPK_CAP];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wave_cnt[TOPK_THREADS / 64];
  __shared__ uint32_t s_gt, s_sel[2];
  const int tid = threadIdx.x;
  const int HW = H * W, N = C * HW;
  const float* img = heat + (size_t)img_i * N;
  const int len = (N + TOPK_SLICES - 1) / TOPK_SLICES;
  const int lo = min(slice * len, N), hi = min(lo + len, N);
  uint64_t* out = out_keys + ((size_t)img_i * TOPK_SLICES + slice) * K;
  const int n = hi - lo;
  if (n <= K) {
    topk_tiny_slice<TOPK_THREADS>(keys, lo, n, K, out, [&](int i) { return f2u(peak_value<NMS>(img, i, H, W)); });
    return;
  }

  // ---- A: lower bound from local maxima
  // (NMS: the 3x3 neighbourhood is only looked at when the raw value could still matter - a
  //  suppressed non-negative element becomes 0 <= raw, so raw <= bound settles it without the 9
  //  loads; negative values, which suppression would RAISE to -0, always take the full path)
  uint32_t lmax = 0;
  {
    int i = lo + tid;
    for (; i + 3 * TOPK_THREADS < hi; i += 4 * TOPK_THREADS) {      // four independent loads in flight
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = img[i + u * TOPK_THREADS];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (!NMS || f2u(v[u]) > lmax || v[u] < 0.0f)
          lmax = max(lmax, NMS ? f2u(peak_value<NMS>(img, i + u * TOPK_THREADS, H, W)) : f2u(v[u]));
    }
    for (; i < hi; i += TOPK_THREADS) {
      const float v = img[i];
      if (!NMS || f2u(v) > lmax || v < 0.0f) lmax = max(lmax, f2u(peak_value<NMS>(img, i, H, W)));
    }
  }
  // K-th largest of the 256 local maxima by rank counting (ties ranked by thread id): one barrier instead of a sort
  uint32_t* lm = reinterpret_cast<uint32_t*>(keys);
  lm[tid] = lmax;
  __syncthreads();
  {
    const u32x4p* l4 = reinterpret_cast<const u32x4p*>(lm);       // (keys[] is 16-byte aligned; eight 16-byte reads in flight)
    int rank = 0;
#pragma unroll 8
    for (int j4 = 0; j4 < TOPK_THREADS / 4; ++j4) {
      const u32x4p o = l4[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) rank += (o[e] > lmax || (o[e] == lmax && 4 * j4 + e < tid)) ? 1 : 0;
    }
    if (rank == K - 1) s_sel[0] = lmax;
  }
  __syncthreads();
  uint32_t L = s_sel[0];
  __syncthreads();

  // ---- B: collect everything strictly above the bound
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (tid == 0) s_gt = 0;
    __syncthreads();
    {
      auto take = [&](int i, float v) {
        uint32_t u = f2u(v);
        if (NMS && (u > L || v < 0.0f)) u = f2u(peak_value<NMS>(img, i, H, W));
        if (u > L) {
          const uint32_t pos = atomicAdd(&s_gt, 1u);
          if (pos < TOPK_CAP) keys[pos] = pack_key(u, i);
        }
      };
      int i = lo + tid;
      for (; i + 3 * TOPK_THREADS < hi; i += 4 * TOPK_THREADS) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = img[i + u * TOPK_THREADS];
#pragma unroll
        for (int u = 0; u < 4; ++u) take(i + u * TOPK_THREADS, v[u]);
      }
      for (; i < hi; i += TOPK_THREADS) take(i, img[i]);
    }
    __syncthreads();
    if (s_gt <= TOPK_CAP) break;
    L = topk_radix_select<TOPK_THREADS>(hist, s_sel, K, [&](auto count) {   // re-reads the slice
      for (int i = lo + tid; i < hi; i += TOPK_THREADS) count(f2u(peak_value<NMS>(img, i, H, W)));
    });
  }
  const int g = (int)s_gt;
  int total = g;
  if (g < K) {
    // index-ordered selection of the (K - g) smallest-index elements equal to L
    const int r = K - g;
    int found = 0;
    for (int base = lo; base < hi && found < r; base += TOPK_THREADS) {
      const int i = base + tid;
      const bool eq = (i < hi) && (!NMS || f2u(img[i]) >= L || img[i] < 0.0f) && (f2u(peak_value<NMS>(img, i, H, W)) == L);
      int all;
      const int rank = found + topk_tie_round<TOPK_THREADS>(eq, wave_cnt, all);
      if (eq && rank < r) keys[g + rank] = pack_key(L, i);
      found += all;
      __syncthreads();
    }
    total = K;
  }
  if (total <= 4 * TOPK_THREADS) {
    __syncthreads();
    rank_select_desc(keys, total, K, out);
    return;
  }
  int P = 1;
  while (P < total) P <<= 1;
  for (int i = total + tid; i < P; i += TOPK_THREADS) keys[i] = 0;
  __syncthreads();
  bitonic_sort_desc(keys, P);
  for (int j = tid; j < K; j += TOPK_THREADS) out[j] = keys[j];
}

template <bool NMS>
__global__ __launch_bounds__(TOPK_THREADS) void topk_slice_kernel(const float* __restrict__ heat, int C, int H,
                                                                  int W, int K, uint64_t* __restrict__ out_keys) {
  topk_slice_body<NMS>(heat, C, H, W, K, out_keys, blockIdx.x / TOPK_SLICES, blockIdx.x % TOPK_SLICES);
}

// Pass 1, register-cached form (maps of up to TOPK_RT * TOPK_RE elements per slice - every map of the 448 x 800 configurations):
// 1024 threads per slice, each holds its <= 16 elements in registers, so the map is read ONCE with every load of the slice
// in flight at the same time (the 256-thread kernel above walks the slice twice, four loads per thread at a time: 14 + 14
// dependent rounds of memory latency per launch - 35 us of the chain between the two head launches).  Same algorithm,
// same keys: A. lower bound L = the K-th largest of G GROUP maxima (a group = 1024 / G neighbouring threads: G >= K distinct
// elements, so at least K elements are >= L); B. everything above L into LDS - from the registers; ties / plateaus and the
// adversarial case exactly as above, on the registers; C. rank counting.
// the LDS of a register-cached slice workgroup (one per kernel: the fused kernel's two selections run on the same one)
struct TopkRegLds {
  uint64_t keys[TOPK_CAP];
  __attribute__((aligned(16))) uint32_t gmax[256];
  uint32_t hist[256];
  uint32_t wave_cnt[TOPK_RT / 64];
  uint32_t s_gt, s_sel[2];
};

// steps A - C on the registers: u[e] = the order-preserving score of flat element lo + tid + e * TOPK_RT (0 past `hi`) of a
// slice of more than K elements -> its K largest as sorted keys in out[0 .. K).  Whole workgroup of TOPK_RT threads.
__device__ __forceinline__ void topk_reg_select(TopkRegLds& s, const uint32_t (&u)[TOPK_RE], int lo, int hi, int K,
                                                uint64_t* __restrict__ out) {
  uint64_t* const keys = s.keys;
  uint32_t* const gmax = s.gmax;
  uint32_t* const hist = s.hist;
  uint32_t* const wave_cnt = s.wave_cnt;
  uint32_t& s_gt = s.s_gt;
  uint32_t* const s_sel = s.s_sel;
  const int tid = threadIdx.x;
  uint32_t lmax = 0;
#pragma unroll
  for (int e = 0; e < TOPK_RE; ++e) lmax = max(lmax, u[e]);
  // ---- A: the K-th largest of the G group maxima (ties ranked by group id).  G = 128 groups of 8 neighbouring threads for
  //      K <= 128, else 256 groups of 4: the rank counting is G^2 compares of VALU work per workgroup - 65,536 of them at
  //      G = 256 were 7 of this kernel's 18 us - and every candidate's count is split over the 1024 / G threads of its group.
  const int P = K <= 128 ? 8 : 4, G = TOPK_RT / P;
  {
    uint32_t m = lmax;
    m = max(m, (uint32_t)__shfl_xor((int)m, 1));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2));
    if (P == 8) m = max(m, (uint32_t)__shfl_xor((int)m, 4));
    if ((tid & (P - 1)) == 0) gmax[tid / P] = m;
  }
  if (tid == 0) s_sel[0] = 0u;                   // (fewer than K non-empty groups - a slice of < P K elements: everything is taken)
  __syncthreads();
  {
    const int c = tid / P, part = tid & (P - 1), per = G / P;      // candidate c against entries [part * per, (part + 1) * per)
    const uint32_t mine = gmax[c];
    const u32x4p* g4 = reinterpret_cast<const u32x4p*>(gmax + part * per);
    int rank = 0;
#pragma unroll 4
    for (int j4 = 0; j4 < per / 4; ++j4) {
      const u32x4p o = g4[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) rank += (o[e] > mine || (o[e] == mine && part * per + 4 * j4 + e < c)) ? 1 : 0;
    }
    rank += __shfl_xor(rank, 1);
    rank += __shfl_xor(rank, 2);
    if (P == 8) rank += __shfl_xor(rank, 4);
    if (part == 0 && rank == K - 1) s_sel[0] = mine;
  }
  __syncthreads();
  uint32_t L = s_sel[0];
  __syncthreads();

  // ---- B0 (the common case): everything >= the bound - at least K elements - fits the candidate buffer: rank counting over
  //      them orders ties at L by index as well (the key's low word), so no tie pass is needed (it cost 8 barrier-separated
  //      rounds on average: 8 of this kernel's 18 us).  A plateau at L (a clamped map) overflows the buffer and takes B below.
  if (tid == 0) s_gt = 0;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < TOPK_RE; ++e) {
    const int i = lo + tid + e * TOPK_RT;
    if (i < hi && u[e] >= L) {
      const uint32_t pos = atomicAdd(&s_gt, 1u);
      if (pos < TOPK_CAP) keys[pos] = pack_key(u[e], i);
    }
  }
  __syncthreads();
  if (s_gt <= TOPK_CAP) {
    rank_select_desc(keys, (int)s_gt, K, out);
    return;
  }
  __syncthreads();

  // ---- B: collect everything strictly above the bound
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (tid == 0) s_gt = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < TOPK_RE; ++e) {
      const int i = lo + tid + e * TOPK_RT;
      if (i < hi && u[e] > L) {
        const uint32_t pos = atomicAdd(&s_gt, 1u);
        if (pos < TOPK_CAP) keys[pos] = pack_key(u[e], i);
      }
    }
    __syncthreads();
    if (s_gt <= TOPK_CAP) break;
    L = topk_radix_select<TOPK_RT>(hist, s_sel, K, [&](auto count) {      // walks the registers
#pragma unroll
      for (int e = 0; e < TOPK_RE; ++e)
        if (lo + tid + e * TOPK_RT < hi) count(u[e]);
    });
  }
  const int g = (int)s_gt;
  int total = g;
  if (g < K) {
    // index-ordered selection of the (K - g) smallest-index elements equal to L
    const int r = K - g;
    int found = 0;
#pragma unroll 1
    for (int e = 0; e < TOPK_RE && found < r; ++e) {
      const int i = lo + tid + e * TOPK_RT;
      uint32_t ue = 0;
#pragma unroll
      for (int q = 0; q < TOPK_RE; ++q) ue = q == e ? u[q] : ue;       // (register array: a select chain, no scratch)
      const bool eq = i < hi && ue == L;
      int all;
      const int rank = found + topk_tie_round<TOPK_RT>(eq, wave_cnt, all);
      if (eq && rank < r) keys[g + rank] = pack_key(L, i);
      found += all;
      __syncthreads();
    }
    total = K;
  }
  __syncthreads();
  rank_select_desc(keys, total, K, out);         // (total <= TOPK_CAP = 4 * TOPK_RT)
}

__global__ __launch_bounds__(TOPK_RT) void topk_slice_reg_kernel(const float* __restrict__ heat, int C, int H, int W, int K,
                                                                 uint64_t* __restrict__ out_keys) {
  __shared__ TopkRegLds s;
  const int tid = threadIdx.x;
  const int N = C * H * W;
  const int img_i = blockIdx.x / TOPK_SLICES, slice = blockIdx.x % TOPK_SLICES;
  const float* img = heat + (size_t)img_i * N;
  const int len = (N + TOPK_SLICES - 1) / TOPK_SLICES;
  const int lo = min(slice * len, N), hi = min(lo + len, N);
  uint64_t* out = out_keys + (size_t)blockIdx.x * K;
  const int n = hi - lo;
  if (n <= K) {
    topk_tiny_slice<TOPK_RT>(s.keys, lo, n, K, out, [&](int i) { return f2u(img[i]); });
    return;
  }
  // element e of this thread = lo + tid + e * TOPK_RT: for a fixed e the threads walk the slice in index order
  uint32_t u[TOPK_RE];
#pragma unroll
  for (int e = 0; e < TOPK_RE; ++e) {
    const int i = lo + tid + e * TOPK_RT;
    u[e] = i < hi ? f2u(img[i]) : 0u;          // (0 ranks below every float but one NaN pattern; validity is tested by index)
  }
  topk_reg_select(s, u, lo, hi, K, out);
}

// The register-cached form with the 3x3 equality NMS inside, and optionally BOTH lists from one read (cf_topk_peaks_fused: the
// index pass of an at-peaks forward, which runs in line and alone on the chip - 1024-thread workgroups find their room).  An
// element's NMS'd score is peak_value<true> of its position - what nms_kernel writes, so the keys are those of the two-pass
// form - from nine loads at clamped window coordinates (at a border the clamp repeats a row / column of the window: the max
// does not change), TOPK_NB elements = 36 loads in flight at a time (16 x 9 values do not fit the 128 registers of a
// 1024-thread workgroup).  The centre value is the raw score.  RAW: the raw list is selected first, then - same LDS - the
// NMS'd one; the slice lists of the raw set lie at out_keys, those of the NMS'd set `set_stride` keys behind.
constexpr int TOPK_NB = 4;
template <bool RAW>
__global__ __launch_bounds__(TOPK_RT) void topk_slice_reg_nms_kernel(const float* __restrict__ heat, int C, int H, int W, int K,
                                                                     uint64_t* __restrict__ out_keys, size_t set_stride) {
  __shared__ TopkRegLds s;
  const int tid = threadIdx.x;
  const int HW = H * W, N = C * HW;
  const int img_i = blockIdx.x / TOPK_SLICES, slice = blockIdx.x % TOPK_SLICES;
  const float* img = heat + (size_t)img_i * N;
  const int len = (N + TOPK_SLICES - 1) / TOPK_SLICES;
  const int lo = min(slice * len, N), hi = min(lo + len, N);
  uint64_t* out_raw = out_keys + (size_t)blockIdx.x * K;
  uint64_t* out_nms = out_raw + set_stride;
  const int n = hi - lo;
  if (n <= K) {
    if (RAW) {
      topk_tiny_slice<TOPK_RT>(s.keys, lo, n, K, out_raw, [&](int i) { return f2u(img[i]); });
      __syncthreads();                         // (the sorted keys are read out: the next sort rewrites them)
    }
    topk_tiny_slice<TOPK_RT>(s.keys, lo, n, K, out_nms, [&](int i) { return f2u(peak_value<true>(img, i, H, W)); });
    return;
  }
  uint32_t ur[TOPK_RE], un[TOPK_RE];                  // (!RAW: ur is never read)
#pragma unroll
  for (int eb = 0; eb < TOPK_RE; eb += TOPK_NB) {
    float w[TOPK_NB][9];
#pragma unroll
    for (int q = 0; q < TOPK_NB; ++q) {
      const int i = min(lo + tid + (eb + q) * TOPK_RT, hi - 1);      // (past the slice: a valid address, the value is dropped)
      const int c = i / HW, pix = i - c * HW;
      const int y = pix / W, x = pix - y * W;
      const float* pl = img + (size_t)c * HW;
      const int r0 = (y > 0 ? y - 1 : y) * W, r1 = y * W, r2 = (y < H - 1 ? y + 1 : y) * W;
      const int x0 = x > 0 ? x - 1 : x, x2 = x < W - 1 ? x + 1 : x;
      w[q][0] = pl[r0 + x0]; w[q][1] = pl[r0 + x]; w[q][2] = pl[r0 + x2];
      w[q][3] = pl[r1 + x0]; w[q][4] = pl[r1 + x]; w[q][5] = pl[r1 + x2];
      w[q][6] = pl[r2 + x0]; w[q][7] = pl[r2 + x]; w[q][8] = pl[r2 + x2];
    }
#pragma unroll
    for (int q = 0; q < TOPK_NB; ++q) {
      const bool in = lo + tid + (eb + q) * TOPK_RT < hi;
      const float v = w[q][4];
      float m = v;
#pragma unroll
      for (int k = 0; k < 9; ++k) m = fmaxf(m, w[q][k]);
      un[eb + q] = in ? f2u((m == v) ? v : v * 0.0f) : 0u;
      ur[eb + q] = in ? f2u(v) : 0u;
    }
  }
  if constexpr (RAW) {
    topk_reg_select(s, ur, lo, hi, K, out_raw);
    __syncthreads();                           // (the last ranking pass reads the candidates: the next selection rewrites them)
  }
  topk_reg_select(s, un, lo, hi, K, out_nms);
}

// the K merged keys of image b -> scores / pixel / class (whole workgroup of THREADS)
template <int THREADS>
__device__ __forceinline__ void emit_peaks(const uint64_t* best, int K, int HW, int b, float* __restrict__ scores,
                                           int32_t* __restrict__ inds, int32_t* __restrict__ classes) {
  for (int j = threadIdx.x; j < K; j += THREADS) {
    float score;
    int pix, cls;
    unpack_key(best[j], HW, score, pix, cls);
    scores[(size_t)b * K + j] = score;
    inds[(size_t)b * K + j] = pix;
    classes[(size_t)b * K + j] = cls;
  }
}

// Pass 2: merge the TOPK_SLICES sorted key lists of one image and emit scores / pixel / class.
__global__ __launch_bounds__(TOPK_MERGE_THREADS) void topk_merge_kernel(const uint64_t* __restrict__ in_keys,
                                                                        int K, int HW, float* __restrict__ scores,
                                                                        int32_t* __restrict__ inds,
                                                                        int32_t* __restrict__ classes) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];      // topk_merge_lds_bytes(K)
  const int tid = threadIdx.x, total = TOPK_SLICES * K;
  const uint64_t* src = in_keys + (size_t)blockIdx.x * total;
  for (int i = tid; i < total; i += TOPK_MERGE_THREADS) keys[i] = src[i];
  __syncthreads();
  emit_peaks<TOPK_MERGE_THREADS>(merge_sorted_lists(keys, keys + total, K), K, HW, blockIdx.x, scores, inds, classes);
}

// Pass 2 of cf_topk_peaks_fused: grid = B x (the sets present), workgroup (b, set) merges the slice lists of image b of its
// set (0 = raw: keys at in_keys, 1 = NMS'd: set_stride keys behind; raw.scores == nullptr: the NMS'd set alone) and emits
// scores / pixel / class - and the entries of cf_head_fused_at's slot tables that come from its list, as
// head_slot_tables_kernel (cf_heads.hip) writes them: tab_ab [B][ceil(2K / 18) * 18] = raw list | NMS'd list | -1,
// tab_b [B][ceil(K / 18) * 18] = NMS'd list | -1, an entry = b * HW + pixel.  The NMS'd set's workgroup writes the padding
// (and, without a raw set, -1 where the raw list would stand).
struct TopkPeakOut {
  float* scores;
  int32_t* inds;
  int32_t* classes;
};
__global__ __launch_bounds__(TOPK_MERGE_THREADS) void topk_merge_fused_kernel(const uint64_t* __restrict__ in_keys, size_t set_stride,
                                                                              int B, int K, int HW, TopkPeakOut raw, TopkPeakOut nms,
                                                                              int32_t* __restrict__ tab_ab, int32_t* __restrict__ tab_b) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];      // topk_merge_lds_bytes(K)
  const int tid = threadIdx.x, total = TOPK_SLICES * K;
  const bool has_raw = raw.scores != nullptr;
  const int b = blockIdx.x % B, set = has_raw ? blockIdx.x / B : 1;
  const uint64_t* src = in_keys + (size_t)set * set_stride + (size_t)b * total;
  for (int i = tid; i < total; i += TOPK_MERGE_THREADS) keys[i] = src[i];
  __syncthreads();
  const uint64_t* best = merge_sorted_lists(keys, keys + total, K);
  const TopkPeakOut o = set ? nms : raw;
  constexpr int slots = CF_HEAD_AT_SLOTS;
  const int per_p = (2 * K + slots - 1) / slots * slots, per_s = (K + slots - 1) / slots * slots;
  int32_t* const tp = tab_ab ? tab_ab + (size_t)b * per_p : nullptr;
  int32_t* const ts = tab_b ? tab_b + (size_t)b * per_s : nullptr;
  for (int j = tid; j < K; j += TOPK_MERGE_THREADS) {
    float score;
    int pix, cls;
    unpack_key(best[j], HW, score, pix, cls);
    o.scores[(size_t)b * K + j] = score;
    o.inds[(size_t)b * K + j] = pix;
    o.classes[(size_t)b * K + j] = cls;
    const int v = (unsigned)pix < (unsigned)HW ? b * HW + pix : -1;
    if (tp) tp[set * K + j] = v;
    if (ts && set) ts[j] = v;
  }
  if (set) {
    if (tp) {
      for (int j = 2 * K + tid; j < per_p; j += TOPK_MERGE_THREADS) tp[j] = -1;
      if (!has_raw)
        for (int j = tid; j < K; j += TOPK_MERGE_THREADS) tp[j] = -1;
    }
    if (ts)
      for (int j = K + tid; j < per_s; j += TOPK_MERGE_THREADS) ts[j] = -1;
  }
}
}  // namespace

static int topk_check_geometry(const char* who, int B, int C, int H, int W, int K) {
  CF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  CF_REQUIRE(K >= 1 && K <= TOPK_MAXK, "%s: K=%d outside [1,%d]", who, K, TOPK_MAXK);
  CF_REQUIRE((long)C * H * W >= K, "%s: fewer than K elements per image", who);
  CF_REQUIRE((long)C * H * W < (1L << 31), "%s: image too large", who);
  return CF_OK;
}

int topk_launch_slices(const char* who, const float* heat, int B, int C, int H, int W, int K, int nms, void* workspace,
                       hipStream_t st) {
  if (const int e = topk_check_geometry(who, B, C, H, W, K)) return e;
  CF_REQUIRE(nms >= 0 && nms <= 2, "%s: nms=%d", who, nms);
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  if (nms == 2) {   // suppressed map first (scratch behind the keys), then the plain top-K over it
    float* sup = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + ((cf_topk_workspace_bytes(B, K) + 255) / 256) * 256);
    const long total = (long)B * C * H * W;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(nms_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, heat, sup, H, W, total);
    heat = sup;
  }
  // (the register-cached kernel - 1024 threads and 35 KB of LDS per workgroup - for the plain top-K, which sits alone on the chip
  //  between the two head launches; behind the NMS pass - the decoder's top-K, issued BESIDE the secondary head launch - the
  //  256-thread kernel, whose workgroups find room next to the head workgroups: the big ones waited for the whole launch)
  const long slice_len = ((long)C * H * W + TOPK_SLICES - 1) / TOPK_SLICES;
  const bool reg = nms == 0 && slice_len <= (long)TOPK_RT * TOPK_RE;
  const auto kernel = reg ? topk_slice_reg_kernel : nms == 1 ? topk_slice_kernel<true> : topk_slice_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(B * TOPK_SLICES), dim3(reg ? TOPK_RT : TOPK_THREADS), 0, st, heat, C, H, W, K, keys);
  return CF_OK;
}

extern "C" size_t cf_topk_workspace_bytes(int B, int K) {
  return (size_t)(B > 0 ? B : 0) * TOPK_SLICES * (size_t)(K > 0 ? K : 0) * sizeof(uint64_t);
}

extern "C" size_t cf_topk_workspace_bytes_nms(int B, int C, int H, int W, int K) {
  const size_t map = (size_t)(B > 0 ? B : 0) * (size_t)(C > 0 ? C : 0) * (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0);
  return ((cf_topk_workspace_bytes(B, K) + 255) / 256) * 256 + map * sizeof(float);
}

extern "C" int cf_topk_peaks(const float* heat, int B, int C, int H, int W, int K, int nms, float* scores,
                             int32_t* inds, int32_t* classes, void* workspace, void* stream) {
  CF_REQUIRE(heat && scores && inds && classes && workspace, "cf_topk_peaks: null buffer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = topk_launch_slices("cf_topk_peaks", heat, B, C, H, W, K, nms, workspace, st)) return e;
  static CfLdsLimit merge_limit;
  merge_limit.ensure(topk_merge_kernel, topk_merge_lds_bytes(K), 65536);
  hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(TOPK_MERGE_THREADS), topk_merge_lds_bytes(K), st,
                     static_cast<const uint64_t*>(workspace), K, H * W, scores, inds, classes);
  return cf_check_launch("cf_topk_peaks");
}

// workspace of cf_topk_peaks_fused: [raw slice lists][NMS'd slice lists][long slices only: the suppressed map of the two-pass form]
static bool topk_fused_reg(int C, int H, int W) {
  return ((long)C * H * W + TOPK_SLICES - 1) / TOPK_SLICES <= (long)TOPK_RT * TOPK_RE;
}

extern "C" size_t cf_topk_peaks_fused_workspace_bytes(int B, int C, int H, int W, int K) {
  const bool reg = C > 0 && H > 0 && W > 0 && topk_fused_reg(C, H, W);
  return cf_topk_workspace_bytes(B, K) + (reg ? cf_topk_workspace_bytes(B, K) : cf_topk_workspace_bytes_nms(B, C, H, W, K));
}

extern "C" int cf_topk_peaks_fused(const float* heat, int B, int C, int H, int W, int K, float* raw_scores, int32_t* raw_inds,
                                   int32_t* raw_classes, float* scores, int32_t* inds, int32_t* classes, int32_t* table_ab,
                                   int32_t* table_b, void* workspace, void* stream) {
  const char* who = "cf_topk_peaks_fused";
  CF_REQUIRE(heat && scores && inds && classes && workspace, "%s: null buffer", who);
  const bool raw = raw_scores != nullptr;
  CF_REQUIRE(raw == (raw_inds != nullptr) && raw == (raw_classes != nullptr), "%s: the raw peaks are all three or none", who);
  if (const int e = topk_check_geometry(who, B, C, H, W, K)) return e;
  if (table_ab || table_b) {
    CF_REQUIRE((long)B * H * W < (1L << 31), "%s: B * HW must stay below 2^31 (flat pixels are int32)", who);
    CF_REQUIRE((long)B * (2L * K + CF_HEAD_AT_SLOTS) < (1L << 31), "%s: B * K too large", who);
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t set_stride = (size_t)B * TOPK_SLICES * K;
  uint64_t* keys = static_cast<uint64_t*>(workspace);
  if (topk_fused_reg(C, H, W)) {
    const auto kernel = raw ? topk_slice_reg_nms_kernel<true> : topk_slice_reg_nms_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(B * TOPK_SLICES), dim3(TOPK_RT), 0, st, heat, C, H, W, K, keys, set_stride);
  } else {
    if (raw)
      if (const int e = topk_launch_slices(who, heat, B, C, H, W, K, 0, keys, st)) return e;
    if (const int e = topk_launch_slices(who, heat, B, C, H, W, K, 2, keys + set_stride, st)) return e;
  }
  static CfLdsLimit merge_limit;
  merge_limit.ensure(topk_merge_fused_kernel, topk_merge_lds_bytes(K), 65536);
  hipLaunchKernelGGL(topk_merge_fused_kernel, dim3(B * (raw ? 2 : 1)), dim3(TOPK_MERGE_THREADS), topk_merge_lds_bytes(K), st,
                     static_cast<const uint64_t*>(keys), set_stride, B, K, H * W, TopkPeakOut{raw_scores, raw_inds, raw_classes},
                     TopkPeakOut{scores, inds, classes}, table_ab, table_b);
  return cf_check_launch(who);
}

namespace {
// cf_topk_peaks_if_changed: the NMS'd top-K of image blockIdx.x, start to end in ONE workgroup - but only if the map's checksum
// parts differ from the expected ones (sums[0 .. CK_PARTS) against sums[CK_PARTS .. 2 CK_PARTS)); equal parts: return at once.
// The decoder's guard for peaks that were computed beside the forward (decode.py): the common case costs one near-empty
// launch, the rare one (the caller wrote into the heat map between forward and decode) ~0.3 ms - never a wrong result.
__global__ __launch_bounds__(TOPK_THREADS) void topk_fallback_kernel(const float* __restrict__ heat, int C, int H, int W, int K,
                                                                     uint64_t* __restrict__ keys_ws, float* __restrict__ scores,
                                                                     int32_t* __restrict__ inds, int32_t* __restrict__ classes,
                                                                     const unsigned long long* __restrict__ sums) {
  {
    int diff = 0;
    for (int i = threadIdx.x; i < CK_PARTS; i += TOPK_THREADS) diff |= sums[i] != sums[CK_PARTS + i] ? 1 : 0;
    if (!__syncthreads_or(diff)) return;
  }
  extern __shared__ __attribute__((aligned(16))) uint64_t mkeys[];     // topk_merge_lds_bytes(K)
  const int b = blockIdx.x, tid = threadIdx.x, total = TOPK_SLICES * K;
  for (int sl = 0; sl < TOPK_SLICES; ++sl) {
    topk_slice_body<true>(heat, C, H, W, K, keys_ws, b, sl);
    __syncthreads();                                                   // (the body's LDS is reused by the next slice)
  }
  __threadfence_block();                                               // the lists were written by this workgroup's own threads
  __syncthreads();
  const uint64_t* src = keys_ws + (size_t)b * total;
  for (int i = tid; i < total; i += TOPK_THREADS) mkeys[i] = src[i];
  __syncthreads();
  emit_peaks<TOPK_THREADS>(merge_sorted_lists(mkeys, mkeys + total, K), K, H * W, b, scores, inds, classes);
}
}  // namespace

extern "C" int cf_topk_peaks_if_changed(const float* heat, int B, int C, int H, int W, int K, int nms, float* scores,
                                        int32_t* inds, int32_t* classes, void* workspace,
                                        const unsigned long long* sums, void* stream) {
  CF_REQUIRE(heat && scores && inds && classes && workspace && sums, "cf_topk_peaks_if_changed: null buffer");
  if (const int e = topk_check_geometry("cf_topk_peaks_if_changed", B, C, H, W, K)) return e;
  CF_REQUIRE(nms == 1 || nms == 2, "cf_topk_peaks_if_changed: nms=%d (the guard of the decoder's NMS'd peaks: 1 or 2, same result)", nms);
  static CfLdsLimit limit;
  limit.ensure(topk_fallback_kernel, topk_merge_lds_bytes(K), 65536);
  hipLaunchKernelGGL(topk_fallback_kernel, dim3(B), dim3(TOPK_THREADS), topk_merge_lds_bytes(K), (hipStream_t)stream, heat, C,
                     H, W, K, static_cast<uint64_t*>(workspace), scores, inds, classes, sums);
  return cf_check_launch("cf_topk_peaks_if_changed");
}

namespace {
// position-weighted 64-bit checksum of a buffer of 32-bit words, as CK_PARTS partial sums: part[b] = sum over the words block b
// walks (16-byte groups g = b * 1024 + t, + CK_PARTS * 1024, ...) of word[i] * (odd 32-bit weight of i) mod 2^64 - exact integer
// arithmetic, a fixed partition, so two runs over the same bits give the same parts; sensitive to WHERE a value sits (a plain
// sum is blind to swaps).  No atomics, no zeroing: 4,096 same-address atomics took 50 us, the memset was a launch of its own.
__global__ __launch_bounds__(1024) void checksum64_kernel(const uint32_t* __restrict__ x, long n, unsigned long long* __restrict__ parts) {
  unsigned long long acc = 0ull;
  const long step = (long)CK_PARTS * 1024;
  const long n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;           // 16-byte loads over the aligned body
  const u32x4p* x4 = reinterpret_cast<const u32x4p*>(x);
  for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < n4; i += step) {
    const u32x4p v = x4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      acc += (unsigned long long)v[e] * (unsigned long long)(((uint32_t)(4 * i + e) * 2654435761u) | 1u);
  }
  for (long i = 4 * n4 + (long)blockIdx.x * 1024 + threadIdx.x; i < n; i += step)
    acc += (unsigned long long)x[i] * (unsigned long long)(((uint32_t)i * 2654435761u) | 1u);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, o, 64);
  __shared__ unsigned long long part[16];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0ull;
    for (int w = 0; w < 16; ++w) t += part[w];
    parts[blockIdx.x] = t;
  }
}
}  // namespace

extern "C" int cf_checksum64(const void* x, long n_words, unsigned long long* parts, void* stream) {
  CF_REQUIRE(x && parts && n_words >= 0, "cf_checksum64: null buffer or n_words=%ld", n_words);
  hipLaunchKernelGGL(checksum64_kernel, dim3(CK_PARTS), dim3(1024), 0, (hipStream_t)stream, static_cast<const uint32_t*>(x), n_words, parts);
  return cf_check_launch("cf_checksum64");
}
